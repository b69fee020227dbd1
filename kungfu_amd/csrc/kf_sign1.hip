// kf_sign1.hip — the 1-bit gradient wire (include/kungfu_amd.h "1-bit gradient
// wire"): what phase 1 of a sharded step carries when the
// exchange's gradient wire is "sign1" (1-bit SGD, EF-signSGD, 1-bit Adam /
// LAMB): one sign bit per element, one f32 magnitude per block of 64, and an
// f32 residual that carries what was dropped to the next step.
//
//   [pack: s = g + r; every bucket's world pieces -> sign bits + block scales;
//          r' = s - decoded]
//     -> all-to-all of the packed pieces
//     -> [fold: the world received pieces of this rank's shard, decoded and
//         added in f32 in rank order, /np, one narrowing] -> the shard
//
// A block is 64 consecutive elements: 8 bytes of sign bits (element i of the
// piece is bit i % 8 of byte i / 8) and one f32 scale, the mean of |s| over
// the block, summed as a pairwise tree of adjacent elements. A piece of q
// elements is q / 8 bytes of bits, then q / 64 scales, then zeros up to the
// next 16 bytes: 12 bytes per block, 0.1875 per element. A block whose sum is
// not finite sends the scale word 0x7fc00000 and zero bits, leaves 64
// residuals of +0.0 and decodes to 0x7fc00000 in every element.
//
// The pack kernel. kf_update_batch.hpp's batched launch, one segment per
// (bucket, piece), 256 lanes. A lane owns 8 consecutive elements (kf_mx8.hip's
// loads: two 16-byte non-temporal loads of f32 gradients, one of 16-bit; the
// residual two 16-byte loads in and two stores out, plain, as §25's A/B
// chose), so a block is 8 lanes, half a DPP row, and a wave's tile is 512
// elements = 8 blocks. Which lanes do what:
//   * every lane: its 8 sums s, three tree levels over its 8 magnitudes in
//     registers, then three cross-lane adds (quad_perm [1,0,3,2], quad_perm
//     [2,3,0,1], row_half_mirror) that finish the tree in the definition's
//     order: lanes 2k and 2k + 1, then pairs of lanes, then the two quads.
//     After the first two steps a quad's four lanes hold the same value, so
//     the mirror (lane i reads lane 7 - i) pairs the quads as an xor 4 would.
//     An f32 add is commutative, so all 8 lanes end with the same bits.
//   * every lane: its byte of sign bits, shifted to byte (lane & 3) of a
//     dword and ORed over the quad by the same two quad_perm steps; the other
//     quad's dword comes by row_half_mirror. The block's first lane (lane & 7
//     == 0) stores both as one 8-byte store: 8 lanes of a wave, 64 contiguous
//     bytes. No byte store, no LDS.
//   * the wave's first lane: the 8 scale words, read from the blocks' first
//     lanes with v_readlane into SGPRs, as two 16-byte stores (the scale area
//     starts 8-byte aligned, after q / 8 bytes of bits; a global 16-byte store
//     needs dword alignment only). The last wave of a piece writes what is
//     left of them as 16- or 8-byte stores together with the piece's zero
//     padding: nblk scales and nblk % 4 zero words are always an even number
//     of words. Blocks past the shard's end load nothing, sum to +0 and so
//     supply those zeros.
// A shard that ends inside a tile runs the same code: q % 64 == 0 keeps a
// block inside the shard or outside it as a whole.
//
// The fold kernel. One segment per bucket, 256 lanes, a lane owns 16
// consecutive elements (a quarter of a block): per rank one 2-byte load of
// bits and the block's scale (a dword load the four lanes of a block share),
// 16 integer decodes (scale_bits | bit << 31, or 0x7fc00000 where the scale is
// not finite) added to 16 f32 accumulators. Rank r + 1's bits and scale are
// loaded before rank r's are decoded, as kf_mx8.hip's fold does. A lane reads
// 6 bytes per rank and writes 64 (f32) or 32: almost all traffic is the store,
// so nothing deeper than that one load ahead is built. The epilogue (/np as a
// template parameter, one narrowing, 16-byte stores) is kf_wire_elt.hpp's,
// shared with kf_mx8.hip.
//
// No contraction (the pragma of kf_reduce_kernels.hpp and -ffp-contract=off),
// no LDS, no scratch.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "kf_update_batch.hpp"
#include "kf_wire_elt.hpp"

namespace kf
{
constexpr int kSign1Block    = 256;  // lanes
constexpr int kSign1Blk      = 64;   // elements per scale
constexpr int kSign1PackElts = 8;    // elements per lane, pack: a block is 8 lanes
constexpr int kSign1FoldElts = 16;   // elements per lane, fold: a quarter of a block
constexpr int kSign1Seg      = 32;   // segments per launch
static_assert(kSign1Blk == 8 * kSign1PackElts, "a block is half a DPP row");

typedef unsigned int sign1_u32x2 __attribute__((ext_vector_type(2)));
// the scale area starts 8-byte aligned: 16-byte accesses at dword alignment
typedef u32x4 sign1_u32x4_a4 __attribute__((aligned(4)));

constexpr unsigned kSign1NaN = 0x7fc00000u;  // the scale word of a block that is not finite

constexpr int kDppXor1       = 0xb1;   // quad_perm:[1,0,3,2]
constexpr int kDppXor2       = 0x4e;   // quad_perm:[2,3,0,1]
constexpr int kDppHalfMirror = 0x141;  // row_half_mirror: lane i of 8 reads lane 7 - i

template <int CTRL> __device__ __forceinline__ unsigned sign1_dpp(unsigned v)
{
    return static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, 0xf, 0xf, false));
}
template <int CTRL> __device__ __forceinline__ float sign1_add_dpp(float a)
{
    return __fadd_rn(a, __uint_as_float(sign1_dpp<CTRL>(__float_as_uint(a))));
}

__device__ __forceinline__ bool sign1_finite(unsigned w) { return (w & 0x7f800000u) != 0x7f800000u; }

// ---- pack ---------------------------------------------------------------------
struct Sign1PackSeg {
    const void *src;  // the piece's q elements inside the gradient bucket
    void *dst;        // the piece: q / 8 bytes of bits, q / 64 scales, zeros to the next 16 bytes
    size_t n;         // q
    void *res;        // the piece's q f32 residuals, read and written
};
struct Sign1PackArgs {
    Sign1PackSeg seg[kSign1Seg];
    unsigned blk0[kSign1Seg + 1];
    int nseg;
};
static_assert(sizeof(Sign1PackArgs) <= 1536, "kernarg budget");

template <typename T>
__device__ __forceinline__ void sign1_pack_body(const Sign1PackSeg &h, size_t blk, size_t nblk)
{
    constexpr int B     = kSign1Block;
    const size_t nunit  = h.n / kSign1PackElts;  // lanes with elements; the bytes of bits
    const size_t nblock = h.n / kSign1Blk;
    const size_t ntiles = (nunit + B - 1) / B;
    char *bits          = static_cast<char *>(h.dst);
    unsigned *scales    = reinterpret_cast<unsigned *>(bits + nunit);
    const unsigned lane = threadIdx.x & 63u;
    // uniform over the workgroup: every lane takes every cross-lane step
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t u    = t * B + threadIdx.x;
        const bool active = u < nunit;  // uniform over a block's 8 lanes: n % 64 == 0
        float s[8];
        wire_load8<T>(h.src, u, active, s);
        u32x4 r0 = {0, 0, 0, 0}, r1 = {0, 0, 0, 0};
        if (active) {
            r0 = ld_u4<0>(h.res, 2 * u);
            r1 = ld_u4<0>(h.res, 2 * u + 1);
        }
        unsigned byte = 0;
        float m[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            s[i]     = __fadd_rn(s[i], __uint_as_float(r0[i]));
            s[4 + i] = __fadd_rn(s[4 + i], __uint_as_float(r1[i]));
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            byte |= (__float_as_uint(s[i]) >> 31) << i;
            m[i] = __uint_as_float(__float_as_uint(s[i]) & 0x7fffffffu);
        }
        // the tree: three levels in registers, three across the block's lanes
        float a = __fadd_rn(__fadd_rn(__fadd_rn(m[0], m[1]), __fadd_rn(m[2], m[3])),
                            __fadd_rn(__fadd_rn(m[4], m[5]), __fadd_rn(m[6], m[7])));
        a = sign1_add_dpp<kDppXor1>(a);
        a = sign1_add_dpp<kDppXor2>(a);
        a = sign1_add_dpp<kDppHalfMirror>(a);
        const bool finite = sign1_finite(__float_as_uint(a));  // a sum of magnitudes: never negative
        const unsigned sc = finite ? __float_as_uint(__fmul_rn(a, 0x1p-6f)) : kSign1NaN;
        if (!finite) byte = 0;

        // r' = s - d, d = the scale with the element's sign
        u32x4 r[2];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float d = __uint_as_float(sc | (__float_as_uint(s[i]) & 0x80000000u));
            r[i / 4][i % 4] = finite ? __float_as_uint(__fsub_rn(s[i], d)) : 0u;
        }
        if (active) {
            st_u4<0>(h.res, 2 * u, r[0]);
            st_u4<0>(h.res, 2 * u + 1, r[1]);
        }

        // the block's 64 bits: this quad's dword, the other quad's, one store
        unsigned w = byte << (8u * (lane & 3u));
        w |= sign1_dpp<kDppXor1>(w);
        w |= sign1_dpp<kDppXor2>(w);
        const unsigned o = sign1_dpp<kDppHalfMirror>(w);
        if (active && (lane & 7u) == 0) reinterpret_cast<sign1_u32x2 *>(bits)[u / 8] = sign1_u32x2{w, o};

        // the wave's 8 scales; blocks past the shard's end have sc == 0
        const int v = static_cast<int>(sc);
        unsigned k[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) k[j] = static_cast<unsigned>(__builtin_amdgcn_readlane(v, 8 * j));
        const size_t b0 = (u & ~static_cast<size_t>(63)) / 8;  // the wave's first block
        if (lane == 0 && b0 < nblock) {
            // words to write: the blocks here, and behind a piece's last block its zero padding
            const size_t left = nblock - b0;
            const unsigned nw = left > 8 ? 8u : static_cast<unsigned>(left + left % 4);  // even, <= 10
            unsigned *p       = scales + b0;
            if (nw >= 4) *reinterpret_cast<sign1_u32x4_a4 *>(p) = u32x4{k[0], k[1], k[2], k[3]};
            else *reinterpret_cast<sign1_u32x2 *>(p) = sign1_u32x2{k[0], k[1]};
            if (nw >= 8) *reinterpret_cast<sign1_u32x4_a4 *>(p + 4) = u32x4{k[4], k[5], k[6], k[7]};
            else if (nw >= 6) *reinterpret_cast<sign1_u32x2 *>(p + 4) = sign1_u32x2{k[4], k[5]};
            if (nw == 10) *reinterpret_cast<sign1_u32x2 *>(p + 8) = sign1_u32x2{0, 0};
        }
    }
}

template <typename T> __global__ void __launch_bounds__(kSign1Block) sign1_pack_ef_kernel(Sign1PackArgs a)
{
    size_t blk, nblk;
    const Sign1PackSeg &g = a.seg[batch_segment(a, blk, nblk)];
    sign1_pack_body<T>(g, blk, nblk);
}

// ---- fold ---------------------------------------------------------------------
struct Sign1FoldSeg {
    const void *pk;  // the world received pieces of this rank's shard, `stride` apart
    void *out;       // the shard, in the bucket's dtype
    size_t n;        // q
    size_t stride;   // kf_sign1_piece_bytes(q)
};
struct Sign1FoldArgs {
    Sign1FoldSeg seg[kSign1Seg];
    unsigned blk0[kSign1Seg + 1];
    int nseg;
};
static_assert(sizeof(Sign1FoldArgs) + sizeof(Div) <= 1536, "kernarg budget");

struct Sign1Raw {
    unsigned bits;   // 16 of them, element i of the lane in bit i
    unsigned scale;  // the block's
};

__device__ __forceinline__ Sign1Raw sign1_fold_load(const char *piece, size_t n, size_t u)
{
    Sign1Raw r;
    r.bits  = reinterpret_cast<const uint16_t *>(piece)[u];
    r.scale = reinterpret_cast<const unsigned *>(piece + n / 8)[u >> 2];
    return r;
}

__device__ __forceinline__ void sign1_decode16(const Sign1Raw &r, float (&v)[16])
{
    const bool finite = sign1_finite(r.scale);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const unsigned d = r.scale | (((r.bits >> i) & 1u) << 31);
        v[i]             = __uint_as_float(finite ? d : kSign1NaN);
    }
}

template <typename T, int DIV>
__device__ __forceinline__ void sign1_fold_body(const Sign1FoldSeg &h, int world, const Div &d,
                                                size_t blk, size_t nblk)
{
    constexpr int B     = kSign1Block;
    const size_t nunit  = h.n / kSign1FoldElts;
    const size_t ntiles = (nunit + B - 1) / B;
    const char *pk      = static_cast<const char *>(h.pk);
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t u = t * B + threadIdx.x;
        if (u >= nunit) continue;
        float acc[16], v[16];
        Sign1Raw cur = sign1_fold_load(pk, h.n, u);
        for (int r = 0; r < world; ++r) {
            Sign1Raw next = cur;
            if (r + 1 < world) next = sign1_fold_load(pk + (r + 1) * h.stride, h.n, u);
            sign1_decode16(cur, v);
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
__global__ void __launch_bounds__(kSign1Block) sign1_fold_kernel(Sign1FoldArgs a, int world, Div np)
{
    size_t blk, nblk;
    const Sign1FoldSeg &g = a.seg[batch_segment(a, blk, nblk)];
    sign1_fold_body<T, DIV>(g, world, np, blk, nblk);
}

}  // namespace kf

namespace
{
using namespace kf;

constexpr UpdateFail fail_pack{"kf_sign1_pack_ef_batch"};
constexpr UpdateFail fail_fold{"kf_sign1_fold_batch"};

size_t piece_bytes(size_t q) { return (q / 8 + q / 16 + 15) / 16 * 16; }

// What both entries check, in kf_mx8_pack_batch's order, before any HIP call;
// q(b): bucket b's shard length.
template <typename Q>
int sign1_check(const UpdateFail &fail, const void *const *a, const void *const *b,
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
        if (q(i) % kSign1Blk) {
            return fail(KF_ERR_ARG, "KF_ERR_ARG", "shard lengths must be multiples of 64 (a block)");
        }
        if (off16(a[i]) || off16(b[i])) return fail(KF_ERR_ARG, "KF_ERR_ARG", kOff16);
    }
    return KF_OK;
}

template <typename T>
int launch_pack(const void *const *grads, void *const *residuals, void *const *packed,
                const size_t *counts, int nb, int world, hipStream_t s)
{
    // one segment per (bucket, piece)
    const size_t W = static_cast<size_t>(world);
    std::vector<size_t> qs(static_cast<size_t>(nb) * W);
    for (size_t i = 0; i < qs.size(); ++i) qs[i] = counts[i / W] / W;
    return plan_update_batch<Sign1PackArgs>(
        qs.data(), static_cast<int>(qs.size()), kSign1PackElts, kSign1Block,
        [&](Sign1PackSeg &g, int i) {
            const size_t b = i / W, j = i % W, q = qs[i];
            g.src = static_cast<const char *>(grads[b]) + j * q * sizeof(typename SgdElt<T>::S);
            g.dst = static_cast<char *>(packed[b]) + j * piece_bytes(q);
            g.n   = q;
            g.res = static_cast<float *>(residuals[b]) + j * q;
        },
        [&](unsigned gx, unsigned gy, const Sign1PackArgs &a) {
            sign1_pack_ef_kernel<T><<<dim3(gx, gy), kSign1Block, 0, s>>>(a);
            return launch_status(fail_pack);
        });
}

template <typename T, int DIV>
int launch_fold(const void *const *packed, void *const *outs, const size_t *q, int nb, int world,
                const Div &dv, hipStream_t s)
{
    return plan_update_batch<Sign1FoldArgs>(
        q, nb, kSign1FoldElts, kSign1Block,
        [&](Sign1FoldSeg &g, int b) {
            g.pk     = packed[b];
            g.out    = outs[b];
            g.n      = q[b];
            g.stride = piece_bytes(q[b]);
        },
        [&](unsigned gx, unsigned gy, const Sign1FoldArgs &a) {
            sign1_fold_kernel<T, DIV><<<dim3(gx, gy), kSign1Block, 0, s>>>(a, world, dv);
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

size_t kf_sign1_piece_bytes(size_t q) { return piece_bytes(q); }

int kf_sign1_pack_ef_batch(const void *const *grads, void *const *residuals, void *const *packed,
                           const size_t *counts, int nb, int world, KungFu_Datatype dt, void *stream)
{
    const UpdateFail &fail = fail_pack;
    const size_t W         = static_cast<size_t>(world);
    int rc = sign1_check(fail, grads, packed, counts, nb, world, dt, 0, [&](int b) { return counts[b] / W; });
    if (rc != KF_OK || nb == 0) return rc;
    if (!residuals) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null table");
    for (int b = 0; b < nb; ++b) {
        if (counts[b] / W == 0) continue;
        if (!residuals[b]) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null residual of a non-empty bucket");
        if (off16(residuals[b])) return fail(KF_ERR_ARG, "KF_ERR_ARG", "residuals must be 16-byte aligned");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dt == KungFu_FLOAT) return launch_pack<float>(grads, residuals, packed, counts, nb, world, s);
    if (dt == KungFu_BFLOAT16) return launch_pack<bf16_t>(grads, residuals, packed, counts, nb, world, s);
    return launch_pack<f16_t>(grads, residuals, packed, counts, nb, world, s);
}

int kf_sign1_fold_batch(const void *const *packed, void *const *out_shards, const size_t *q, int nb,
                        int world, KungFu_Datatype dt, int np, void *stream)
{
    const int rc = sign1_check(fail_fold, packed, out_shards, q, nb, world, dt, np,
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
