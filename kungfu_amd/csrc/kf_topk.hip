// kf_topk.hip — the block-wise top-k gradient wire (include/kungfu_amd.h
// "Top-k gradient wire"): what phase 1 of a sharded step carries
// when the exchange's gradient wire is "topk" (Deep Gradient Compression,
// sparsified SGD with memory): of every block of 64 elements the k largest
// magnitudes of s = g + r with their places, k in {1, 2, 4, 8}, and an f32
// residual that keeps what was not sent.
//
//   [pack: s = g + r; every bucket's world pieces -> per block k values and k
//          index bytes; r' = 0 where sent, s elsewhere]
//     -> all-to-all of the packed pieces
//     -> [fold: the world received pieces of this rank's shard scattered into a
//         zeroed f32 tile in rank order, /np, one narrowing] -> the shard
//
// A piece of q elements (nblk = q / 64 blocks) is nblk * k f32 values, block
// after block in selection order, then nblk * k index bytes (0..63) in the same
// order, then zeros up to the next 16 bytes. An element's key is its magnitude
// bits (bits & 0x7fffffff) as an integer, so NaN and inf order above every
// finite value; among equal keys the smaller index is taken first.
//
// The pack kernel. kf_sign1.hip's work split: one segment per (bucket, piece),
// 256 lanes, a lane owns 8 consecutive elements, a block is 8 lanes (half a DPP
// row), a wave's tile is 8 blocks, all selecting at once. A lane keeps per
// element the key (an int, -1 once the element is taken) and a tag, (the
// element's index in the block) << 1 | its sign bit: tags of different elements
// order as their indices do. Round j of K:
//   * every lane: the best of its 8 (key, tag), a strict > scan in index order,
//     so ties keep the smaller index. A lane has at most j < 8 taken elements,
//     so its best is never a taken one.
//   * the block's 8 lanes: three cross-lane steps (quad_perm [1,0,3,2],
//     quad_perm [2,3,0,1], row_half_mirror), each a lexicographic choice:
//     larger key, then smaller tag. Tags are distinct, so both sides of a step
//     choose the same pair; after the two quad steps a quad's lanes agree and
//     the mirror (lane i reads lane 7 - i) pairs the quads as an xor 4 would.
//   * the lane that owns the chosen element sets its key to -1; lane j of the
//     block keeps the value (key | sign << 31: s's bits) and the index.
// Stores: lanes j < K of a block store their value as a dword, 8 K contiguous
// dwords per wave. The index bytes are shifted to byte (lane & 3) of a dword
// and ORed over the lanes that hold them by the same DPP steps; the block's
// first lane stores 8 bytes (K = 8), 4 (K = 4), 2 (K = 2) or 1 (K = 1). The
// wave that holds a piece's last block writes the zero padding, one lane per
// 8, 4, 2 or 1 bytes of it. Residuals: two 16-byte loads in and two stores
// out per lane, plain, as §25's A/B chose.
//
// The fold kernel. One segment per bucket, 256 lanes, a workgroup's tile is
// 1024 output elements (16 blocks) as f32 in LDS. Every lane zeroes the 4
// elements it will read out; a barrier; then per rank the tile's 16 K entries
// are contiguous in both areas of the piece: lane e < 16 K loads entry e (a
// dword and a byte) and adds it into LDS at 64 (e / K) + (index & 63). 64 is a
// multiple of K, so the entries of a block belong to one wave for every rank:
// rank order is that wave's program order and no barrier stands between
// ranks. Rank r + 1's entry is loaded before rank r's is added. A barrier,
// then every lane reads its 4 elements back and stores them through
// kf_wire_elt.hpp's epilogue. A piece that names one index twice in a (rank,
// block) is malformed: one of the two adds is lost, nothing is written
// outside the block.
//
// No contraction (the pragma of kf_reduce_kernels.hpp and -ffp-contract=off),
// no scratch, no atomics; the pack uses no LDS.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "kf_update_batch.hpp"
#include "kf_wire_elt.hpp"

namespace kf
{
constexpr int kTopkBlock    = 256;   // lanes
constexpr int kTopkBlk      = 64;    // elements per block
constexpr int kTopkPackElts = 8;     // elements per lane, pack: a block is 8 lanes
constexpr int kTopkFoldElts = 4;     // elements per lane, the fold's read-out
constexpr int kTopkFoldTile = kTopkBlock * kTopkFoldElts;  // 1024 elements = 16 blocks in LDS
constexpr int kTopkSeg      = 32;    // segments per launch
static_assert(kTopkBlk == 8 * kTopkPackElts, "a block is half a DPP row");

constexpr int kTopkDppXor1       = 0xb1;   // quad_perm:[1,0,3,2]
constexpr int kTopkDppXor2       = 0x4e;   // quad_perm:[2,3,0,1]
constexpr int kTopkDppHalfMirror = 0x141;  // row_half_mirror: lane i of 8 reads lane 7 - i

template <int CTRL> __device__ __forceinline__ unsigned topk_dpp(unsigned v)
{
    return static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, 0xf, 0xf, false));
}
// one cross-lane step of the selection: the larger key, then the smaller tag
template <int CTRL> __device__ __forceinline__ void topk_agree(int &key, unsigned &tag)
{
    const int ko      = static_cast<int>(topk_dpp<CTRL>(static_cast<unsigned>(key)));
    const unsigned to = topk_dpp<CTRL>(tag);
    const bool other  = ko > key || (ko == key && to < tag);
    key               = other ? ko : key;
    tag               = other ? to : tag;
}

// ---- pack ---------------------------------------------------------------------
struct TopkPackSeg {
    const void *src;  // the piece's q elements inside the gradient bucket
    void *dst;        // the piece: q / 64 * K values, as many index bytes, zeros to the next 16 bytes
    size_t n;         // q
    void *res;        // the piece's q f32 residuals, read and written
};
struct TopkPackArgs {
    TopkPackSeg seg[kTopkSeg];
    unsigned blk0[kTopkSeg + 1];
    int nseg;
};
static_assert(sizeof(TopkPackArgs) <= 1536, "kernarg budget");

// what one lane stores of the index area and of the padding: 8, 4, 2 or 1 bytes
template <int K> struct TopkIdxUnit;
template <> struct TopkIdxUnit<8> { using U = wire_u32x2; };
template <> struct TopkIdxUnit<4> { using U = unsigned; };
template <> struct TopkIdxUnit<2> { using U = uint16_t; };
template <> struct TopkIdxUnit<1> { using U = uint8_t; };

template <typename T, int K>
__device__ __forceinline__ void topk_pack_body(const TopkPackSeg &h, size_t blk, size_t nblk)
{
    using U             = typename TopkIdxUnit<K>::U;
    constexpr int B     = kTopkBlock;
    const size_t nunit  = h.n / kTopkPackElts;  // lanes with elements
    const size_t nblock = h.n / kTopkBlk;
    const size_t ntiles = (nunit + B - 1) / B;
    unsigned *vals      = static_cast<unsigned *>(h.dst);
    char *idx           = static_cast<char *>(h.dst) + nblock * K * sizeof(float);
    const unsigned lane = threadIdx.x & 63u;
    const unsigned bl   = lane & 7u;  // the lane's place in its block
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
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            s[i]     = __fadd_rn(s[i], __uint_as_float(r0[i]));
            s[4 + i] = __fadd_rn(s[4 + i], __uint_as_float(r1[i]));
        }
        int key[8];       // the magnitude bits; -1 once the element is taken
        unsigned tag[8];  // (index in the block) << 1 | sign
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            key[i] = static_cast<int>(__float_as_uint(s[i]) & 0x7fffffffu);
            tag[i] = ((8u * bl + i) << 1) | (__float_as_uint(s[i]) >> 31);
        }
        unsigned value = 0, index = 0;  // lane j < K of the block: round j's
#pragma unroll
        for (int j = 0; j < K; ++j) {
            int k      = key[0];
            unsigned w = tag[0];
#pragma unroll
            for (int i = 1; i < 8; ++i) {
                const bool better = key[i] > k;
                k                 = better ? key[i] : k;
                w                 = better ? tag[i] : w;
            }
            topk_agree<kTopkDppXor1>(k, w);
            topk_agree<kTopkDppXor2>(k, w);
            topk_agree<kTopkDppHalfMirror>(k, w);
            const unsigned e    = w >> 1;                         // the block's choice
            const unsigned mine = (e >> 3) == bl ? (e & 7u) : 8u;  // which of this lane's, if any
#pragma unroll
            for (int i = 0; i < 8; ++i) key[i] = mine == static_cast<unsigned>(i) ? -1 : key[i];
            if (bl == static_cast<unsigned>(j)) {
                value = static_cast<unsigned>(k) | (w << 31);
                index = e;
            }
        }

        // r' = +0 where the element was sent or is not finite, s elsewhere
        u32x4 r[2];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned bits = __float_as_uint(s[i]);
            const bool keep     = key[i] >= 0 && (bits & 0x7f800000u) != 0x7f800000u;
            r[i / 4][i % 4]     = keep ? bits : 0u;
        }
        if (active) {
            st_u4<0>(h.res, 2 * u, r[0]);
            st_u4<0>(h.res, 2 * u + 1, r[1]);
        }

        const size_t b = u / 8;  // the lane's block
        if (active && bl < static_cast<unsigned>(K)) vals[b * K + bl] = value;

        // the block's K index bytes in its first lane; lanes past K hold 0
        unsigned w = index << (8u * (lane & 3u));
        if constexpr (K >= 2) w |= topk_dpp<kTopkDppXor1>(w);
        if constexpr (K >= 4) w |= topk_dpp<kTopkDppXor2>(w);
        U out;
        if constexpr (K == 8) out = wire_u32x2{w, topk_dpp<kTopkDppHalfMirror>(w)};
        else out = static_cast<U>(w);
        if (active && bl == 0) reinterpret_cast<U *>(idx)[b] = out;

        // the wave with the piece's last block: zeros up to the next 16 bytes
        const size_t b0 = (u & ~static_cast<size_t>(63)) / 8;  // the wave's first block
        if (b0 < nblock && nblock <= b0 + 8) {
            const size_t end   = nblock * K * 5;  // a multiple of sizeof(U)
            const unsigned pad = static_cast<unsigned>((16 - end % 16) % 16);
            if (lane * sizeof(U) < pad) {
                U zero;
                __builtin_memset(&zero, 0, sizeof(U));
                reinterpret_cast<U *>(static_cast<char *>(h.dst) + end)[lane] = zero;
            }
        }
    }
}

template <typename T, int K> __global__ void __launch_bounds__(kTopkBlock) topk_pack_ef_kernel(TopkPackArgs a)
{
    size_t blk, nblk;
    const TopkPackSeg &g = a.seg[batch_segment(a, blk, nblk)];
    topk_pack_body<T, K>(g, blk, nblk);
}

// ---- fold ---------------------------------------------------------------------
struct TopkFoldSeg {
    const void *pk;  // the world received pieces of this rank's shard, `stride` apart
    void *out;       // the shard, in the bucket's dtype
    size_t n;        // q
    size_t stride;   // kf_topk_piece_bytes(q, K)
};
struct TopkFoldArgs {
    TopkFoldSeg seg[kTopkSeg];
    unsigned blk0[kTopkSeg + 1];
    int nseg;
};
static_assert(sizeof(TopkFoldArgs) + sizeof(Div) <= 1536, "kernarg budget");

struct TopkEntry {
    float value;
    unsigned index;
};

// entry `at` of a piece of nent entries
__device__ __forceinline__ TopkEntry topk_fold_load(const char *piece, size_t nent, size_t at)
{
    TopkEntry e;
    e.value = reinterpret_cast<const float *>(piece)[at];
    e.index = reinterpret_cast<const uint8_t *>(piece + nent * sizeof(float))[at];
    return e;
}

template <typename T, int DIV, int K>
__device__ __forceinline__ void topk_fold_body(const TopkFoldSeg &h, int world, const Div &d, size_t blk,
                                               size_t nblk, float *tile)
{
    constexpr int TB    = kTopkFoldTile / kTopkBlk;  // blocks per tile
    const size_t nblock = h.n / kTopkBlk;
    const size_t nent   = nblock * K;
    const size_t ntiles = (nblock + TB - 1) / TB;
    const char *pk      = static_cast<const char *>(h.pk);
    const unsigned e    = threadIdx.x;
    float4 *mine        = reinterpret_cast<float4 *>(tile) + e;  // what this lane zeroes and reads out
    // uniform over the workgroup: every lane reaches both barriers
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t left   = nblock - t * TB;
        const unsigned here = static_cast<unsigned>(left < TB ? left : TB) * K;  // the tile's entries per rank
        *mine               = float4{0.0f, 0.0f, 0.0f, 0.0f};
        __syncthreads();  // another wave scatters into this lane's 4
        if (e < here) {
            const size_t at = t * TB * K + e;
            float *slot     = tile + kTopkBlk * (e / K);
            TopkEntry cur   = topk_fold_load(pk, nent, at);
            for (int r = 0; r < world; ++r) {
                TopkEntry next = cur;
                if (r + 1 < world) next = topk_fold_load(pk + (r + 1) * h.stride, nent, at);
                float *p = slot + (cur.index & 63u);
                *p       = __fadd_rn(*p, cur.value);
                // a block's entries are this wave's for every rank: program order is rank order
                __builtin_amdgcn_wave_barrier();
                cur = next;
            }
        }
        __syncthreads();
        const float4 v = *mine;
        float acc[4]   = {v.x, v.y, v.z, v.w};
        const size_t u = t * kTopkBlock + e;  // 4 elements; n % 64 == 0 keeps them whole
        if (u * kTopkFoldElts < h.n) wire_store4<T, DIV>(h.out, u, acc, d);
    }
}

template <typename T, int DIV, int K>
__global__ void __launch_bounds__(kTopkBlock) topk_fold_kernel(TopkFoldArgs a, int world, Div np)
{
    __shared__ __attribute__((aligned(16))) float tile[kTopkFoldTile];
    size_t blk, nblk;
    const TopkFoldSeg &g = a.seg[batch_segment(a, blk, nblk)];
    topk_fold_body<T, DIV, K>(g, world, np, blk, nblk, tile);
}

}  // namespace kf

namespace
{
using namespace kf;

constexpr UpdateFail fail_pack{"kf_topk_pack_ef_batch"};
constexpr UpdateFail fail_fold{"kf_topk_fold_batch"};

bool good_k(int k) { return k == 1 || k == 2 || k == 4 || k == 8; }
size_t piece_bytes(size_t q, int k) { return (5 * static_cast<size_t>(k) * (q / kTopkBlk) + 15) / 16 * 16; }

// What both entries check, in kf_sign1_pack_ef_batch's order with k behind the
// world, before any HIP call; q(b): bucket b's shard length.
template <typename Q>
int topk_check(const UpdateFail &fail, const void *const *a, const void *const *b, const size_t *counts,
               int nb, int world, KungFu_Datatype dt, int np, int k, Q &&q)
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
    if (!good_k(k)) return fail(KF_ERR_ARG, "KF_ERR_ARG", "k must be 1, 2, 4 or 8");
    if (np < 0) return fail(KF_ERR_ARG, "KF_ERR_ARG", "np < 0");
    for (int i = 0; i < nb; ++i) {
        if (q(i) == 0) continue;
        if (!a[i] || !b[i]) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null pointer in a non-empty bucket");
        if (q(i) % kTopkBlk) {
            return fail(KF_ERR_ARG, "KF_ERR_ARG", "shard lengths must be multiples of 64 (a block)");
        }
        if (off16(a[i]) || off16(b[i])) return fail(KF_ERR_ARG, "KF_ERR_ARG", kOff16);
    }
    return KF_OK;
}

template <typename T, int K>
int launch_pack(const void *const *grads, void *const *residuals, void *const *packed,
                const size_t *counts, int nb, int world, hipStream_t s)
{
    // one segment per (bucket, piece)
    const size_t W = static_cast<size_t>(world);
    std::vector<size_t> qs(static_cast<size_t>(nb) * W);
    for (size_t i = 0; i < qs.size(); ++i) qs[i] = counts[i / W] / W;
    return plan_update_batch<TopkPackArgs>(
        qs.data(), static_cast<int>(qs.size()), kTopkPackElts, kTopkBlock,
        [&](TopkPackSeg &g, int i) {
            const size_t b = i / W, j = i % W, q = qs[i];
            g.src = static_cast<const char *>(grads[b]) + j * q * sizeof(typename SgdElt<T>::S);
            g.dst = static_cast<char *>(packed[b]) + j * piece_bytes(q, K);
            g.n   = q;
            g.res = static_cast<float *>(residuals[b]) + j * q;
        },
        [&](unsigned gx, unsigned gy, const TopkPackArgs &a) {
            topk_pack_ef_kernel<T, K><<<dim3(gx, gy), kTopkBlock, 0, s>>>(a);
            return launch_status(fail_pack);
        });
}

template <typename T, int DIV, int K>
int launch_fold(const void *const *packed, void *const *outs, const size_t *q, int nb, int world,
                const Div &dv, hipStream_t s)
{
    return plan_update_batch<TopkFoldArgs>(
        q, nb, kTopkFoldElts, kTopkBlock,
        [&](TopkFoldSeg &g, int b) {
            g.pk     = packed[b];
            g.out    = outs[b];
            g.n      = q[b];
            g.stride = piece_bytes(q[b], K);
        },
        [&](unsigned gx, unsigned gy, const TopkFoldArgs &a) {
            topk_fold_kernel<T, DIV, K><<<dim3(gx, gy), kTopkBlock, 0, s>>>(a, world, dv);
            return launch_status(fail_fold);
        });
}

template <typename T, int K>
int launch_fold_div(const void *const *packed, void *const *outs, const size_t *q, int nb,
                    int world, int np, hipStream_t s)
{
    const Div dv = update_div(np);
    switch (update_div_code(np, dv)) {
    case 0: return launch_fold<T, 0, K>(packed, outs, q, nb, world, dv, s);
    case 1: return launch_fold<T, 1, K>(packed, outs, q, nb, world, dv, s);
    default: return launch_fold<T, 2, K>(packed, outs, q, nb, world, dv, s);
    }
}

// f(std::integral_constant<int, K>) for the host's k (checked: 1, 2, 4 or 8)
template <typename F> int with_k(int k, F &&f)
{
    switch (k) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 8>{});
    }
}

}  // namespace

extern "C" {

size_t kf_topk_piece_bytes(size_t q, int k) { return good_k(k) ? piece_bytes(q, k) : 0; }

int kf_topk_pack_ef_batch(const void *const *grads, void *const *residuals, void *const *packed,
                          const size_t *counts, int nb, int world, KungFu_Datatype dt, int k,
                          void *stream)
{
    const UpdateFail &fail = fail_pack;
    const size_t W         = static_cast<size_t>(world);
    int rc = topk_check(fail, grads, packed, counts, nb, world, dt, 0, k, [&](int b) { return counts[b] / W; });
    if (rc != KF_OK || nb == 0) return rc;
    if (!residuals) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null table");
    for (int b = 0; b < nb; ++b) {
        if (counts[b] / W == 0) continue;
        if (!residuals[b]) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null residual of a non-empty bucket");
        if (off16(residuals[b])) return fail(KF_ERR_ARG, "KF_ERR_ARG", "residuals must be 16-byte aligned");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_k(k, [&](auto K) {
        if (dt == KungFu_FLOAT) return launch_pack<float, decltype(K)::value>(grads, residuals, packed, counts, nb, world, s);
        if (dt == KungFu_BFLOAT16) {
            return launch_pack<bf16_t, decltype(K)::value>(grads, residuals, packed, counts, nb, world, s);
        }
        return launch_pack<f16_t, decltype(K)::value>(grads, residuals, packed, counts, nb, world, s);
    });
}

int kf_topk_fold_batch(const void *const *packed, void *const *out_shards, const size_t *q, int nb,
                       int world, KungFu_Datatype dt, int np, int k, void *stream)
{
    const int rc = topk_check(fail_fold, packed, out_shards, q, nb, world, dt, np, k,
                              [&](int b) { return q[b]; });
    if (rc != KF_OK || nb == 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_k(k, [&](auto K) {
        if (dt == KungFu_FLOAT) return launch_fold_div<float, decltype(K)::value>(packed, out_shards, q, nb, world, np, s);
        if (dt == KungFu_BFLOAT16) {
            return launch_fold_div<bf16_t, decltype(K)::value>(packed, out_shards, q, nb, world, np, s);
        }
        return launch_fold_div<f16_t, decltype(K)::value>(packed, out_shards, q, nb, world, np, s);
    });
}

}  // extern "C"
