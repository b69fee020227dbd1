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
// Two more pack kernels, mx8_pack_ef_kernel (error feedback: a f32 residual
// carried from step to step) and mx8_pack_sr_kernel (stochastic rounding with
// Philox draws), share the pack's skeleton; they are described where they
// stand, and in DESIGN.md §25. The format, the fold and the plain pack are
// the same under all three.
//
// No contraction (the pragma of kf_reduce_kernels.hpp and -ffp-contract=off),
// no LDS, no scratch.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "kf_philox.hpp"
#include "kf_update_batch.hpp"
#include "kf_wire_elt.hpp"

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
        wire_load8<T>(h.src, u, active, x);
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

// ---- pack with error feedback, pack with stochastic rounding --------------------
// mx8_pack_body's skeleton (tiles, quads, the scale byte, both stores, the
// shard that ends inside a tile) with another element step each.
//
// Error feedback (EF-SGD, 1-bit Adam): s = widen(g) + r with the f32 residual
// r of the same bucket index, scale and codes from s as mx8_pack_body makes
// them from g, d = the codes unpacked in registers (v_cvt_scalef32_pk_f32_fp8
// on the two code dwords the lane is about to store), r' = s - d stored over
// r. A block that is not finite (scale byte 0xFF) leaves 32 residuals of
// +0.0. The residual moves as two 16-byte loads and two 16-byte stores per
// lane; the policy is KF_MX8_EF_R_NT / KF_MX8_EF_ST_NT (DESIGN.md §25 has the
// A/B): 8 more bytes per element than the plain pack. The gradients are only
// read.
//
// Stochastic rounding. The scale byte is the plain pack's. With y = x * 2^-e
// (one v_ldexp_f32: exact unless y is an f32 subnormal, far below what any
// draw can lift to a code), t = |y| and a 16-bit draw r16:
//   t >= 2^-6: code_mag = ((bits(t) + (r16 << 4)) >> 20) - 960
//   t <  2^-6: code_mag = (trunc_u32(t * 2^29) + (r16 << 4)) >> 20   (0 .. 8)
//   code = sign(x) << 7 | code_mag
// 20 mantissa bits are dropped either way (below 2^-6 the unit is E4M3's
// subnormal step 2^-9, so t * 2^29 counts it in 2^-20ths), r16 << 4 is a
// uniform 20-bit addend with four zero bits below, and a value that is an
// E4M3 value at its scale has those 20 bits zero: it is returned whatever the
// draw. The block's largest element is below 448, so rounding up ends at 448
// (0x7e), never at the NaN code. Plain integer ALU; the hardware's *_sr_*
// conversions were not taken.
//
// The draws are a pure function of (seed, step, rank, bucket index, element
// index in the bucket); launch geometry and the segment split play no part.
// The host folds the first four into two words per bucket,
//   w = splitmix64(splitmix64(splitmix64(seed) ^ step) ^ (rank << 32 | bucket))
//   key = low32(w), c1 = high32(w)
// and one Philox2x32-10 evaluation serves the four consecutive elements
// 4c .. 4c + 3 of the bucket: (a, b) = philox2x32_10(c0 = c, c1, key), draws
// a >> 16, a & 0xffff, b >> 16, b & 0xffff. A lane's 8 elements start at a
// multiple of 8 (pieces are whole blocks), so it makes two evaluations.
#ifndef KF_MX8_EF_R_NT
#define KF_MX8_EF_R_NT 0  // the residual's loads, 1 = non-temporal
#endif
#ifndef KF_MX8_EF_ST_NT
#define KF_MX8_EF_ST_NT 0  // the residual's stores
#endif

struct Mx8EfSeg {
    const void *src;  // as Mx8PackSeg
    void *dst;
    size_t n;
    void *res;  // the piece's q f32 residuals, read and written
};
struct Mx8SrSeg {
    const void *src;
    void *dst;
    size_t n;
    uint64_t base;         // the bucket index of the piece's first element, a multiple of 32
    uint32_t key, stream;  // Philox key and counter word c1 of the bucket
};
template <typename SEG> struct Mx8VarArgs {
    SEG seg[kMx8Seg];
    unsigned blk0[kMx8Seg + 1];
    int nseg;
};
static_assert(sizeof(Mx8VarArgs<Mx8SrSeg>) <= 1536, "kernarg budget");

// one element's code under the draw r16 < 2^16; nege = -e. The arm that is
// not taken converts a clamped t, so that the conversion is always in range.
__device__ __forceinline__ unsigned mx8_sr_code(float x, int nege, uint32_t r16)
{
    const unsigned b = __float_as_uint(ldexpf(x, nege));
    const unsigned t = b & 0x7fffffffu, r = r16 << 4;
    const unsigned normal = ((t + r) >> 20) - 960u;
    const unsigned sub    = (static_cast<unsigned>(__uint_as_float(min(t, 0x3c800000u)) * 0x1p29f) + r) >> 20;
    return ((b >> 31) << 7) | (t >= 0x3c800000u ? normal : sub);
}

// four elements, the bucket's elements 4 * c0 .. 4 * c0 + 3 -> four codes in a dword
__device__ __forceinline__ unsigned mx8_sr4(const float *x, int nege, uint32_t c0, const Mx8SrSeg &h)
{
    const Philox2 p = philox2x32_10(c0, h.stream, h.key);
    return mx8_sr_code(x[0], nege, p.a >> 16) | (mx8_sr_code(x[1], nege, p.a & 0xffffu) << 8) |
           (mx8_sr_code(x[2], nege, p.b >> 16) << 16) | (mx8_sr_code(x[3], nege, p.b & 0xffffu) << 24);
}

template <typename T, typename SEG>
__device__ __forceinline__ void mx8_pack_var_body(const SEG &h, size_t blk, size_t nblk)
{
    constexpr bool EF   = std::is_same<SEG, Mx8EfSeg>::value;
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
        wire_load8<T>(h.src, u, active, x);
        if constexpr (EF) {
            u32x4 r0 = {0, 0, 0, 0}, r1 = {0, 0, 0, 0};
            if (active) {
                r0 = ld_u4<KF_MX8_EF_R_NT>(h.res, 2 * u);
                r1 = ld_u4<KF_MX8_EF_R_NT>(h.res, 2 * u + 1);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                x[i]     = __fadd_rn(x[i], __uint_as_float(r0[i]));
                x[4 + i] = __fadd_rn(x[4 + i], __uint_as_float(r1[i]));
            }
        }
        unsigned mag = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) mag = max(mag, __float_as_uint(x[i]) & 0x7fffffffu);
        const unsigned byte = mx8_scale_byte(mx8_quad_max(mag));
        const float scale   = __uint_as_float(byte << 23);  // the instructions read the exponent field
        mx8_u32x2 out;
        if constexpr (EF) {
            out = mx8_u32x2{mx8_cvt4(x[0], x[1], x[2], x[3], scale),
                            mx8_cvt4(x[4], x[5], x[6], x[7], scale)};
        } else {
            const int nege    = 127 - static_cast<int>(byte);
            const uint32_t c0 = static_cast<uint32_t>((h.base + u * kMx8PackElts) >> 2);
            out = mx8_u32x2{mx8_sr4(x, nege, c0, h), mx8_sr4(x + 4, nege, c0 + 1, h)};
        }
        if (byte == 0xffu) out = mx8_u32x2{0, 0};
        const u32x4 sc = mx8_wave_scales(byte);
        if (active) reinterpret_cast<mx8_u32x2 *>(codes)[u] = out;
        const size_t uw = u & ~static_cast<size_t>(63);  // the wave's first unit
        if ((threadIdx.x & 63u) == 0 && uw < nunit) st_u4<0>(scales, uw / 64, sc);
        if constexpr (EF) {
            u32x4 r[2];
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const f32x2 lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(out[w], scale, false);
                const f32x2 hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(out[w], scale, true);
                r[w] = u32x4{__float_as_uint(__fsub_rn(x[4 * w], lo.x)),
                             __float_as_uint(__fsub_rn(x[4 * w + 1], lo.y)),
                             __float_as_uint(__fsub_rn(x[4 * w + 2], hi.x)),
                             __float_as_uint(__fsub_rn(x[4 * w + 3], hi.y))};
                if (byte == 0xffu) r[w] = u32x4{0, 0, 0, 0};
            }
            if (active) {
                st_u4<KF_MX8_EF_ST_NT>(h.res, 2 * u, r[0]);
                st_u4<KF_MX8_EF_ST_NT>(h.res, 2 * u + 1, r[1]);
            }
        }
    }
}

template <typename T> __global__ void __launch_bounds__(kMx8Block) mx8_pack_ef_kernel(Mx8VarArgs<Mx8EfSeg> a)
{
    size_t blk, nblk;
    const Mx8EfSeg &g = a.seg[batch_segment(a, blk, nblk)];
    mx8_pack_var_body<T>(g, blk, nblk);
}

template <typename T> __global__ void __launch_bounds__(kMx8Block) mx8_pack_sr_kernel(Mx8VarArgs<Mx8SrSeg> a)
{
    size_t blk, nblk;
    const Mx8SrSeg &g = a.seg[batch_segment(a, blk, nblk)];
    mx8_pack_var_body<T>(g, blk, nblk);
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
        wire_store16<T, DIV>(h.out, u, acc, d);
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
constexpr UpdateFail fail_pack_ef{"kf_mx8_pack_ef_batch"};
constexpr UpdateFail fail_pack_sr{"kf_mx8_pack_sr_batch"};
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

// The pack variants: launch_pack's segments, `fill(seg, b, j, q)` adding what
// the variant's segment holds beyond src, dst and n.
template <typename T, typename SEG, typename KERNEL, typename FILL>
int launch_pack_var(const UpdateFail &fail, KERNEL kernel, const void *const *grads,
                    void *const *packed, const size_t *counts, int nb, int world, hipStream_t s,
                    FILL &&fill)
{
    const size_t W = static_cast<size_t>(world);
    std::vector<size_t> qs(static_cast<size_t>(nb) * W);
    for (size_t i = 0; i < qs.size(); ++i) qs[i] = counts[i / W] / W;
    return plan_update_batch<Mx8VarArgs<SEG>>(
        qs.data(), static_cast<int>(qs.size()), kMx8PackElts, kMx8Block,
        [&](SEG &g, int i) {
            const size_t b = i / W, j = i % W, q = qs[i];
            g.src = static_cast<const char *>(grads[b]) + j * q * sizeof(typename SgdElt<T>::S);
            g.dst = static_cast<char *>(packed[b]) + j * piece_bytes(q);
            g.n   = q;
            fill(g, b, j, q);
        },
        [&](unsigned gx, unsigned gy, const Mx8VarArgs<SEG> &a) {
            kernel<<<dim3(gx, gy), kMx8Block, 0, s>>>(a);
            return launch_status(fail);
        });
}

template <typename T>
int launch_pack_ef(const void *const *grads, void *const *residuals, void *const *packed,
                   const size_t *counts, int nb, int world, hipStream_t s)
{
    return launch_pack_var<T, Mx8EfSeg>(
        fail_pack_ef, mx8_pack_ef_kernel<T>, grads, packed, counts, nb, world, s,
        [&](Mx8EfSeg &g, size_t b, size_t j, size_t q) {
            g.res = static_cast<float *>(residuals[b]) + j * q;
        });
}

template <typename T>
int launch_pack_sr(const void *const *grads, void *const *packed, const size_t *counts, int nb,
                   int world, uint64_t seed, uint64_t step, int rank, int bucket0, hipStream_t s)
{
    const uint64_t at = splitmix64(splitmix64(seed) ^ step);
    return launch_pack_var<T, Mx8SrSeg>(
        fail_pack_sr, mx8_pack_sr_kernel<T>, grads, packed, counts, nb, world, s,
        [&](Mx8SrSeg &g, size_t b, size_t j, size_t q) {
            const uint64_t bucket = static_cast<uint32_t>(bucket0) + b;
            const uint64_t w = splitmix64(at ^ (static_cast<uint64_t>(rank) << 32 | bucket));
            g.base   = j * q;
            g.key    = static_cast<uint32_t>(w);
            g.stream = static_cast<uint32_t>(w >> 32);
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

int kf_mx8_pack_ef_batch(const void *const *grads, void *const *residuals, void *const *packed,
                         const size_t *counts, int nb, int world, KungFu_Datatype dt, void *stream)
{
    const UpdateFail &fail = fail_pack_ef;
    const size_t W         = static_cast<size_t>(world);
    int rc = mx8_check(fail, grads, packed, counts, nb, world, dt, 0, [&](int b) { return counts[b] / W; });
    if (rc != KF_OK || nb == 0) return rc;
    if (!residuals) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null table");
    for (int b = 0; b < nb; ++b) {
        if (counts[b] / W == 0) continue;
        if (!residuals[b]) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null residual of a non-empty bucket");
        if (off16(residuals[b])) return fail(KF_ERR_ARG, "KF_ERR_ARG", "residuals must be 16-byte aligned");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dt == KungFu_FLOAT) return launch_pack_ef<float>(grads, residuals, packed, counts, nb, world, s);
    if (dt == KungFu_BFLOAT16) {
        return launch_pack_ef<bf16_t>(grads, residuals, packed, counts, nb, world, s);
    }
    return launch_pack_ef<f16_t>(grads, residuals, packed, counts, nb, world, s);
}

int kf_mx8_pack_sr_batch(const void *const *grads, void *const *packed, const size_t *counts, int nb,
                         int world, KungFu_Datatype dt, uint64_t seed, uint64_t step, int rank,
                         int bucket0, void *stream)
{
    const UpdateFail &fail = fail_pack_sr;
    const int rc = mx8_check(fail, grads, packed, counts, nb, world, dt, 0,
                             [&](int b) { return counts[b] / static_cast<size_t>(world); });
    if (rc != KF_OK || nb == 0) return rc;
    if (rank < 0 || rank >= world) return fail(KF_ERR_ARG, "KF_ERR_ARG", "rank must be in [0, world)");
    if (bucket0 < 0) return fail(KF_ERR_ARG, "KF_ERR_ARG", "bucket0 < 0");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dt == KungFu_FLOAT) {
        return launch_pack_sr<float>(grads, packed, counts, nb, world, seed, step, rank, bucket0, s);
    }
    if (dt == KungFu_BFLOAT16) {
        return launch_pack_sr<bf16_t>(grads, packed, counts, nb, world, seed, step, rank, bucket0, s);
    }
    return launch_pack_sr<f16_t>(grads, packed, counts, nb, world, seed, step, rank, bucket0, s);
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
