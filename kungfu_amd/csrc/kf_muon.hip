// kf_muon.hip — Muon on the sharded step (include/kungfu_amd.h "Muon",
// DESIGN.md §28): momentum on the shard, an all-gather of bf16 directions,
// and on every rank an orthogonalised update of every weight matrix by a
// quintic Newton-Schulz iteration,
//
//   X = d / (|d|_F + 1e-7)
//   5 times:  A = X X^T ;  B = b*A + c*A*A ;  X = a*X + B*X
//   p = p*(1 - lr*wd) - lr*sqrt(max(1, rows/cols)) * X
//
// whose hot path is three matrix products per iteration and tensor. They are
// three launches of ONE grouped GEMM kernel over all the tensors of a bucket
// group, the library's first use of CDNA4's matrix instructions.
//
// muon_gemm_kernel:  C_i = alpha*Cin_i + beta*op(A_i)*op(B_i), bf16 in, f32
// accumulation in v_mfma_f32_32x32x16_bf16, one narrowing to bf16.
//
//   * Work split. A block of 256 lanes (four waves, 2 x 2) owns one 64 x 64
//     tile of one problem's C (one tile per block) and walks K in steps of 32; a wave owns a
//     32 x 32 quadrant: one accumulator of 16 VGPRs, two MFMAs per K step.
//     A block finds (problem, tile) with kf_update_batch.hpp's lookup over the
//     prefix table of the problems' tile counts, 32 problems per launch.
//   * Data movement. Per K step the block reads a 64 x 32 piece of op(A) and
//     of op(B): 256 chunks of 8 elements each, one per lane and operand, as
//     one 16-byte load where the chunk lies inside the matrix and the
//     operand's base and leading dimension are multiples of 16 bytes, else as
//     eight predicated 2-byte loads with zeros outside (ragged M, N and K, and
//     tensors that start anywhere in a bucket, take this path; the choice is
//     per chunk, there is no host-side special case). Both operands sit in LDS
//     K-major, As[m][k] and Bs[n][k], which is how the MFMA wants them: lane l
//     supplies row (l % 32), k = 8 * (l / 32) .. + 7 of either operand as ONE
//     16-byte LDS read. An operand stored the other way round (X^T of a tall
//     tensor's X^T X, and every NN product's B) is transposed on its way into
//     LDS: the lane's 8 elements go to 8 rows. Rows are padded from 64 to 80
//     bytes, so the 32 rows a half-wave reads start in different banks.
//   * Pipeline. Two LDS buffers: the next K step's chunks are loaded into
//     registers before the MFMAs of the current one and stored into the other
//     buffer after them; one barrier per K step.
//   * Epilogue. Lane l holds column (l % 32) and rows 8*(j/4) + 4*(l/32) + j%4
//     (j = 0..15) of its quadrant: alpha*Cin + beta*acc as three f32
//     operations, one RNE narrowing, a masked 2-byte store.
//   * No atomics, no split-K, no inline asm: every C element is one lane's sum
//     in a fixed order, so the result is a pure function of the inputs.
//
// muon_syrk_kernel:  C_i = alpha*Cin_i + beta*S_i*S_i^T with S = op(A_i), the
// two products of an iteration whose result is symmetric (A = X X^T, and
// B = b*A + c*A*A = b*A + c*A*A^T), opt-in (kf_muon_syrk_grouped).
//
//   * Work split. Only the tiles (ti, tj), tj <= ti, of the T x T grid of
//     64 x 64 tiles are launched: T(T+1)/2 blocks a problem, the prefix table
//     counts those, and a block turns its linear index into (ti, tj) with a
//     float square root and an integer correction (muon_tri).
//   * Operands. Both MFMA operands are row panels of S, rows 64*ti.. as the
//     first and rows 64*tj.. as the second, in the general kernel's K-major
//     LDS layout and K order: for row >= col the accumulator is the general
//     kernel's NT (TN) accumulator bit for bit. A diagonal tile stages ONE
//     panel a K step and reads both fragments from it. (Its quadrant above
//     the diagonal is computed and dropped: a wave-uniform branch round the
//     MFMAs costs 16 VGPRs of accumulator copies and two waves per SIMD.)
//     With A stored m x k there is no 2-byte LDS store at all; stored k x m,
//     both panels are transposed on their way in as the general kernel does it.
//   * Epilogue through LDS. After the K walk's last barrier the operand
//     buffers are free: every lane narrows its 16 elements (Cin read only
//     where row >= col) into a 64 x 64 bf16 tile whose rows are 33 dwords
//     apart, so the 8 lanes that gather one transposed row read LDS rows 8
//     apart, which start 8 banks apart. An off-diagonal tile leaves LDS twice, row-wise to (ti, tj) and
//     column-wise to (tj, ti); a diagonal one once, out[r][c] =
//     lds[max(r, c)][min(r, c)]. The upper half of C is therefore a copy of
//     the lower one's bits, never a second computation. Stores are 16-byte
//     chunks where the chunk lies inside C and c and ldc are multiples of 16
//     bytes, masked 2-byte stores otherwise, chosen per chunk.
//
// Not done: a larger block tile for large matrices, and the
// general kernel's epilogue through LDS.
//
// The element-wise kernels. muon_momentum_kernel is kf_sgd.hip's shape on the
// shard (16-byte vectors, 8 elements per lane: f32 g and m in, f32 m and bf16
// d out). muon_scale_kernel and muon_apply_kernel run over whole tensors
// where they lie in their buckets, which is at any element, so they move one
// element per lane and access: 2- and 4-byte accesses, coalesced.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "kf_sgd_elt.hpp"
#include "kf_update_batch.hpp"

namespace kf
{
constexpr int kMuonSeg   = 32;
constexpr int kMuonBlock = 256;
constexpr int kMuonTile  = 64;  // C tile of a block, both ways (kf_muon_tile)
constexpr int kMuonBK    = 32;            // K step
constexpr int kMuonLd    = kMuonBK + 8;   // LDS row in elements: 80 bytes
constexpr int kMuonEltTile = 4 * kMuonBlock;  // elements of a tile of scale / apply
constexpr int kMuonMomUnit = 8;               // elements a lane of the momentum kernel owns

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct MuonGemmSeg {
    const uint16_t *a, *b, *cin;
    uint16_t *c;
    int m, n, k;
    int lda, ldb, ldcin, ldc;
    // bit 0: A stored K x M, bit 1: B stored N x K, bits 2, 3: a, b take 16-byte loads,
    // bit 4 (muon_syrk_kernel, which reads no b and no n): c takes 16-byte stores
    int flags;
};
struct MuonGemmArgs {
    MuonGemmSeg seg[kMuonSeg];
    unsigned blk0[kMuonSeg + 1];
    int nseg;
};
static_assert(sizeof(MuonGemmSeg) == 64, "kernarg entry");
static_assert(sizeof(MuonGemmArgs) + 2 * sizeof(float) <= 3072, "kernarg budget");

// Elements (r, c .. c + 7) of a row-major R x C matrix, zeros outside it.
__device__ __forceinline__ u32x4 muon_ld8(const uint16_t *p, int ld, int r, int c, int R, int C,
                                          bool vec)
{
    u32x4 v = {0u, 0u, 0u, 0u};
    if (r >= R || c >= C) return v;
    const uint16_t *q = p + static_cast<size_t>(r) * ld + c;
    if (vec && c + 8 <= C) return *reinterpret_cast<const u32x4 *>(q);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t e = (c + i < C) ? q[i] : 0u;
        v[i / 2] |= e << (16 * (i & 1));
    }
    return v;
}

// A lane's chunk of one operand's 64 x 32 piece at (row0, k0), and its way
// into LDS. kmajor: the operand is stored [row][k] (rows x K, ld): chunk t
// is row t / 4, k = 8 * (t % 4) .. + 7, one 16-byte LDS store. Otherwise it is
// stored [k][row] (K x rows, ld): chunk t is k = t / 8, rows 8 * (t % 8) .. + 7,
// eight 2-byte LDS stores.
__device__ __forceinline__ u32x4 muon_fetch(const uint16_t *p, int ld, bool kmajor, bool vec,
                                            int row0, int rows, int k0, int K)
{
    const int t = threadIdx.x;
    if (kmajor) return muon_ld8(p, ld, row0 + (t >> 2), k0 + 8 * (t & 3), rows, K, vec);
    return muon_ld8(p, ld, k0 + (t >> 3), row0 + 8 * (t & 7), K, rows, vec);
}

__device__ __forceinline__ void muon_stage(uint16_t *lds, bool kmajor, const u32x4 &v)
{
    const int t = threadIdx.x;
    if (kmajor) {
        *reinterpret_cast<u32x4 *>(lds + (t >> 2) * kMuonLd + 8 * (t & 3)) = v;
    } else {
        uint16_t *q = lds + 8 * (t & 7) * kMuonLd + (t >> 3);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            q[i * kMuonLd] = static_cast<uint16_t>(v[i / 2] >> (16 * (i & 1)));
        }
    }
}

__global__ void __launch_bounds__(kMuonBlock)
    muon_gemm_kernel(MuonGemmArgs args, float alpha, float beta)
{
    static_assert(kMuonTile == 64 && kMuonBlock == 256, "four waves, 2 x 2 quadrants of 32 x 32");
    __shared__ __attribute__((aligned(16))) uint16_t lds[2][2][kMuonTile * kMuonLd];
    size_t blk, nblk;
    const MuonGemmSeg &h = args.seg[batch_segment(args, blk, nblk)];
    const int M = h.m, N = h.n, K = h.k;
    const unsigned tn     = (N + kMuonTile - 1) / kMuonTile;
    const unsigned ntiles = (M + kMuonTile - 1) / kMuonTile * tn;  // the host keeps it below 2^31
    const bool amajor = !(h.flags & 1), bmajor = (h.flags & 2) != 0;
    const bool avec = (h.flags & 4) != 0, bvec = (h.flags & 8) != 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = 32 * (wave >> 1), wn = 32 * (wave & 1);
    const int frag = (lane & 31) * kMuonLd + 8 * (lane >> 5);  // the lane's row and k offset
    const int nk = (K + kMuonBK - 1) / kMuonBK;

    // one tile per block (the host refuses a problem of more tiles than a
    // grid row holds); a row's blocks past the problem's last tile leave
    const unsigned t = static_cast<unsigned>(blk);
    if (t >= ntiles) return;
    const int m0 = static_cast<int>(t / tn) * kMuonTile, n0 = static_cast<int>(t % tn) * kMuonTile;
    f32x16 acc;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0f;

    u32x4 ra = muon_fetch(h.a, h.lda, amajor, avec, m0, M, 0, K);
    u32x4 rb = muon_fetch(h.b, h.ldb, bmajor, bvec, n0, N, 0, K);
    muon_stage(lds[0][0], amajor, ra);
    muon_stage(lds[0][1], bmajor, rb);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) {
            ra = muon_fetch(h.a, h.lda, amajor, avec, m0, M, (kt + 1) * kMuonBK, K);
            rb = muon_fetch(h.b, h.ldb, bmajor, bvec, n0, N, (kt + 1) * kMuonBK, K);
        }
#pragma unroll
        for (int kk = 0; kk < kMuonBK; kk += 16) {
            const u32x4 fa = *reinterpret_cast<const u32x4 *>(&lds[cur][0][wm * kMuonLd + frag + kk]);
            const u32x4 fb = *reinterpret_cast<const u32x4 *>(&lds[cur][1][wn * kMuonLd + frag + kk]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa),
                                                          __builtin_bit_cast(bf16x8, fb), acc, 0, 0, 0);
        }
        if (kt + 1 < nk) {
            muon_stage(lds[cur ^ 1][0], amajor, ra);
            muon_stage(lds[cur ^ 1][1], bmajor, rb);
        }
        __syncthreads();
    }

    const int col = n0 + wn + (lane & 31);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int row = m0 + wm + 8 * (j / 4) + 4 * (lane >> 5) + (j % 4);
        if (row < M && col < N) {
            float v = __fmul_rn(beta, acc[j]);
            if (h.cin) {
                const float x = bf16_to_f32(h.cin[static_cast<size_t>(row) * h.ldcin + col]);
                v             = __fadd_rn(__fmul_rn(alpha, x), v);
            }
            h.c[static_cast<size_t>(row) * h.ldc + col] = f32_to_bf16(v);
        }
    }
}

// ---- the symmetric product -------------------------------------------------------
constexpr int kMuonLdC = kMuonTile + 2;  // the epilogue tile's LDS row in elements: 33 dwords

// Elements (r, c .. c + 7) of v into a row-major M x M matrix, nothing outside it.
__device__ __forceinline__ void muon_st8(uint16_t *p, int ld, int r, int c, int M, bool vec,
                                         const u32x4 &v)
{
    if (r >= M || c >= M) return;
    uint16_t *q = p + static_cast<size_t>(r) * ld + c;
    if (vec && c + 8 <= M) {
        *reinterpret_cast<u32x4 *>(q) = v;
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (c + i < M) q[i] = static_cast<uint16_t>(v[i / 2] >> (16 * (i & 1)));
    }
}

// Tile t of a lower triangle counted row by row -> (ti, tj), tj <= ti:
// ti = the largest i with i (i + 1) / 2 <= t. The float estimate can be off
// by one from 8 t + 1 >= 2^24 on; the integer steps make it exact for every t
// (the host admits t < 2^22, so ti < 2896 and nothing here overflows).
__device__ __forceinline__ void muon_tri(unsigned t, int &ti, int &tj)
{
    unsigned i = static_cast<unsigned>((sqrtf(8.0f * static_cast<float>(t) + 1.0f) - 1.0f) * 0.5f);
    while (i * (i + 1) / 2 > t) --i;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    ti = static_cast<int>(i);
    tj = static_cast<int>(t - i * (i + 1) / 2);
}

__global__ void __launch_bounds__(kMuonBlock)
    muon_syrk_kernel(MuonGemmArgs args, float alpha, float beta)
{
    static_assert(kMuonTile == 64 && kMuonBlock == 256, "four waves, 2 x 2 quadrants of 32 x 32");
    static_assert(kMuonTile * kMuonLdC <= 4 * kMuonTile * kMuonLd, "the epilogue tile fits");
    __shared__ __attribute__((aligned(16))) uint16_t lds[2][2][kMuonTile * kMuonLd];
    size_t blk, nblk;
    const MuonGemmSeg &h = args.seg[batch_segment(args, blk, nblk)];
    const int M = h.m, K = h.k;
    const unsigned tm = (M + kMuonTile - 1) / kMuonTile;
    const unsigned t  = static_cast<unsigned>(blk);
    if (t >= tm * (tm + 1) / 2) return;  // a row's blocks past the problem's last tile
    int ti, tj;
    muon_tri(t, ti, tj);
    const bool diag = ti == tj;
    const bool kmajor = !(h.flags & 1), avec = (h.flags & 4) != 0, cvec = (h.flags & 16) != 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = 32 * (wave >> 1), wn = 32 * (wave & 1);
    const int m0 = ti * kMuonTile, n0 = tj * kMuonTile;
    const int frag = (lane & 31) * kMuonLd + 8 * (lane >> 5);
    const int nk = (K + kMuonBK - 1) / kMuonBK;
    const int second = diag ? 0 : 1;  // the LDS panel of the second operand
    f32x16 acc;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0f;

    u32x4 ra = muon_fetch(h.a, h.lda, kmajor, avec, m0, M, 0, K);
    u32x4 rb = {0u, 0u, 0u, 0u};
    if (!diag) rb = muon_fetch(h.a, h.lda, kmajor, avec, n0, M, 0, K);
    muon_stage(lds[0][0], kmajor, ra);
    if (!diag) muon_stage(lds[0][1], kmajor, rb);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) {
            ra = muon_fetch(h.a, h.lda, kmajor, avec, m0, M, (kt + 1) * kMuonBK, K);
            if (!diag) rb = muon_fetch(h.a, h.lda, kmajor, avec, n0, M, (kt + 1) * kMuonBK, K);
        }
#pragma unroll
        for (int kk = 0; kk < kMuonBK; kk += 16) {
            const u32x4 fa = *reinterpret_cast<const u32x4 *>(&lds[cur][0][wm * kMuonLd + frag + kk]);
            const u32x4 fb =
                *reinterpret_cast<const u32x4 *>(&lds[cur][second][wn * kMuonLd + frag + kk]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa),
                                                          __builtin_bit_cast(bf16x8, fb), acc, 0, 0, 0);
        }
        if (kt + 1 < nk) {
            muon_stage(lds[cur ^ 1][0], kmajor, ra);
            if (!diag) muon_stage(lds[cur ^ 1][1], kmajor, rb);
        }
        __syncthreads();
    }

    // The tile, narrowed, into LDS: the operand buffers are free behind the
    // K walk's last barrier. Rows past M hold zeros that nothing stores, and
    // what a diagonal tile holds above its diagonal is never read.
    uint16_t *e = &lds[0][0][0];
    const int lc = wn + (lane & 31), col = n0 + lc;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int lr = wm + 8 * (j / 4) + 4 * (lane >> 5) + (j % 4), row = m0 + lr;
        float v = __fmul_rn(beta, acc[j]);
        if (h.cin && row < M && col <= row) {
            const float x = bf16_to_f32(h.cin[static_cast<size_t>(row) * h.ldcin + col]);
            v             = __fadd_rn(__fmul_rn(alpha, x), v);
        }
        e[lr * kMuonLdC + lc] = f32_to_bf16(v);
    }
    __syncthreads();
    // 512 chunks of 8 elements, two per lane: chunk q is row q / 8 of what is
    // stored, columns 8 * (q % 8) .. + 7, so 8 lanes fill a row's 128 bytes.
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int q = threadIdx.x + u * kMuonBlock, r = q >> 3, c0 = 8 * (q & 7);
        u32x4 v = {0u, 0u, 0u, 0u};
        if (diag) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = c0 + i, hi = r > c ? r : c, lo = r > c ? c : r;
                v[i / 2] |= static_cast<uint32_t>(e[hi * kMuonLdC + lo]) << (16 * (i & 1));
            }
            muon_st8(h.c, h.ldc, m0 + r, m0 + c0, M, cvec, v);
        } else {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(e + r * kMuonLdC + c0);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = w[i];
            muon_st8(h.c, h.ldc, m0 + r, n0 + c0, M, cvec, v);
            u32x4 x = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                x[i / 2] |= static_cast<uint32_t>(e[(c0 + i) * kMuonLdC + r]) << (16 * (i & 1));
            }
            muon_st8(h.c, h.ldc, n0 + r, m0 + c0, M, cvec, x);
        }
    }
}

// ---- momentum on the shard -----------------------------------------------------
//   g = np > 0 ? sum / np : sum ;  m = (mu*m) + g ;  d = nesterov ? g + (mu*m) : m
struct MuonMomSeg {
    const void *g;
    void *m, *d;
    size_t n;
    float mu;
    int nesterov;
};
struct MuonMomArgs {
    MuonMomSeg seg[kMuonSeg];
    unsigned blk0[kMuonSeg + 1];
    int nseg;
};

template <int DIV>
__device__ __forceinline__ void muon_momentum_body(const MuonMomSeg &h, size_t blk, size_t nblk,
                                                   const Div &np)
{
    const size_t nunit  = h.n / kMuonMomUnit;
    const size_t ntiles = (nunit + kMuonBlock - 1) / kMuonBlock;
    for (size_t t = blk; t < ntiles; t += nblk) {
        const size_t u = t * kMuonBlock + threadIdx.x;
        if (u >= nunit) break;
        u32x4 rg[2], rm[2], rd;
#pragma unroll
        for (int v = 0; v < 2; ++v) rg[v] = ld_u4<1>(h.g, 2 * u + v);
#pragma unroll
        for (int v = 0; v < 2; ++v) rm[v] = ld_u4<0>(h.m, 2 * u + v);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float g = SgdDiv<float, DIV>::run(__uint_as_float(rg[i / 4][i % 4]), np);
            const float m = __fadd_rn(__fmul_rn(h.mu, __uint_as_float(rm[i / 4][i % 4])), g);
            const float d = h.nesterov ? __fadd_rn(g, __fmul_rn(h.mu, m)) : m;
            rm[i / 4][i % 4] = __float_as_uint(m);
            const uint32_t e = f32_to_bf16(d);
            if (i & 1) rd[i / 2] |= e << 16;
            else rd[i / 2] = e;
        }
#pragma unroll
        for (int v = 0; v < 2; ++v) st_u4<0>(h.m, 2 * u + v, rm[v]);
        st_u4<0>(h.d, u, rd);
    }
}

__global__ void __launch_bounds__(kMuonBlock) muon_momentum_kernel(MuonMomArgs a, Div np, int div)
{
    size_t blk, nblk;
    const MuonMomSeg &h = a.seg[batch_segment(a, blk, nblk)];
    dispatch_div(div, [&](auto D) { muon_momentum_body<decltype(D)::value>(h, blk, nblk, np); });
}

// ---- X0 = d * 1 / (|d| + 1e-7), and the parameters' update ------------------------
struct MuonEltSeg {
    void *out;       // scale: bf16 X0; apply: f32 parameters
    const void *in;  // scale: bf16 d; apply: bf16 X
    const double *sq;  // scale: the tensor's squared norm, on the device
    size_t n;
    float dk, nc;  // apply: 1 - lr*wd and -lr*sqrt(max(1, rows/cols))
};
struct MuonEltArgs {
    MuonEltSeg seg[kMuonSeg];
    unsigned blk0[kMuonSeg + 1];
    int nseg;
};

template <bool APPLY> __global__ void __launch_bounds__(kMuonBlock) muon_elt_kernel(MuonEltArgs a)
{
    size_t blk, nblk;
    const MuonEltSeg &h  = a.seg[batch_segment(a, blk, nblk)];
    const uint16_t *in   = static_cast<const uint16_t *>(h.in);
    const size_t ntiles  = (h.n + kMuonEltTile - 1) / kMuonEltTile;
    float s = 0.0f;
    if constexpr (!APPLY) s = static_cast<float>(1.0 / (__dsqrt_rn(*h.sq) + 1e-7));
    for (size_t t = blk; t < ntiles; t += nblk) {
#pragma unroll
        for (int u = 0; u < kMuonEltTile / kMuonBlock; ++u) {
            const size_t i = t * kMuonEltTile + u * kMuonBlock + threadIdx.x;
            if (i >= h.n) break;
            const float x = bf16_to_f32(in[i]);
            if constexpr (APPLY) {
                float *p = static_cast<float *>(h.out);
                p[i]     = __fadd_rn(__fmul_rn(h.dk, p[i]), __fmul_rn(h.nc, x));
            } else {
                static_cast<uint16_t *>(h.out)[i] = f32_to_bf16(__fmul_rn(x, s));
            }
        }
    }
}

}  // namespace kf

namespace
{
using namespace kf;

constexpr UpdateFail fail_mom{"kf_muon_momentum_batch"};
constexpr UpdateFail fail_scale{"kf_muon_scale_batch"};
constexpr UpdateFail fail_gemm{"kf_muon_gemm_grouped"};
constexpr UpdateFail fail_syrk{"kf_muon_syrk_grouped"};
constexpr UpdateFail fail_apply{"kf_muon_apply_batch"};

bool off(const void *p, uintptr_t align) { return (reinterpret_cast<uintptr_t>(p) % align) != 0; }

// What the element-wise entries check alike: nb, the dtype (wrong: the
// refusal's text), the tables, then per non-empty segment null pointers and
// the pointers' alignment.
template <size_t K>
int muon_check(const UpdateFail &fail, const void *const *const (&tabs)[K],
               const uintptr_t (&align)[K], const void *also, const size_t *counts, int nb,
               const char *wrong = nullptr)
{
    if (nb < 0) return fail(KF_ERR_ARG, "KF_ERR_ARG", "nb < 0");
    if (nb == 0) return KF_OK;
    if (wrong) return fail(KF_ERR_DTYPE, "KF_ERR_DTYPE", wrong);
    bool null = !counts || !also;
    for (const void *const *t : tabs) null = null || !t;
    if (null) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null table");
    for (int b = 0; b < nb; ++b) {
        if (counts[b] == 0) continue;
        bool none = false, bad = false;
        for (size_t i = 0; i < K; ++i) {
            none = none || !tabs[i][b];
            bad  = bad || off(tabs[i][b], align[i]);
        }
        if (none) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null pointer in a non-empty segment");
        if (bad) return fail(KF_ERR_ARG, "KF_ERR_ARG", "misaligned pointer");
    }
    return KF_OK;
}

}  // namespace

extern "C" {

int kf_muon_tile(void) { return kMuonTile; }

int kf_muon_momentum_batch(const void *const *grads, void *const *moms, void *const *dirs,
                           const size_t *counts, int nb, KungFu_Datatype dt, int np,
                           const kf_muon_hyper *hyper, void *stream)
{
    const void *const *const tabs[3] = {grads, moms, dirs};
    const uintptr_t align[3]         = {16, 16, 16};
    const int rc = muon_check(fail_mom, tabs, align, hyper, counts, nb,
                              dt != KungFu_FLOAT ? "f32 gradients and momentum only" : nullptr);
    if (rc != KF_OK || nb == 0) return rc;
    if (np < 0) return fail_mom(KF_ERR_ARG, "KF_ERR_ARG", "np < 0");
    for (int b = 0; b < nb; ++b) {
        if (counts[b] % kMuonMomUnit) {
            return fail_mom(KF_ERR_ARG, "KF_ERR_ARG", "counts must be multiples of 8 elements");
        }
    }
    const Div dv  = update_div(np);
    const int div = update_div_code(np, dv);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return plan_update_batch<MuonMomArgs>(
        counts, nb, kMuonMomUnit, kMuonBlock,
        [&](MuonMomSeg &g, int b) {
            g = MuonMomSeg{grads[b], moms[b], dirs[b], counts[b],
                           static_cast<float>(hyper[b].momentum), hyper[b].nesterov ? 1 : 0};
        },
        [&](unsigned gx, unsigned gy, const MuonMomArgs &a) {
            muon_momentum_kernel<<<dim3(gx, gy), kMuonBlock, 0, s>>>(a, dv, div);
            return launch_status(fail_mom);
        });
}

int kf_muon_scale_batch(const void *const *dirs, void *const *xs, const size_t *counts,
                        const double *sq, int nb, void *stream)
{
    const void *const *const tabs[2] = {dirs, xs};
    const uintptr_t align[2]         = {2, 2};
    const int rc = muon_check(fail_scale, tabs, align, sq, counts, nb);
    if (rc != KF_OK || nb == 0) return rc;
    if (off(sq, 8)) return fail_scale(KF_ERR_ARG, "KF_ERR_ARG", "misaligned pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return plan_update_batch<MuonEltArgs>(
        counts, nb, 1, kMuonEltTile,
        [&](MuonEltSeg &g, int b) { g = MuonEltSeg{xs[b], dirs[b], sq + b, counts[b], 0.0f, 0.0f}; },
        [&](unsigned gx, unsigned gy, const MuonEltArgs &a) {
            muon_elt_kernel<false><<<dim3(gx, gy), kMuonBlock, 0, s>>>(a);
            return launch_status(fail_scale);
        });
}

int kf_muon_apply_batch(void *const *params, const void *const *xs, const size_t *counts,
                        const kf_muon_apply *hyper, int nb, KungFu_Datatype dt, void *stream)
{
    const void *const *const tabs[2] = {params, xs};
    const uintptr_t align[2]         = {4, 2};
    const int rc = muon_check(fail_apply, tabs, align, hyper, counts, nb,
                              dt != KungFu_FLOAT ? "f32 parameters only" : nullptr);
    if (rc != KF_OK || nb == 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return plan_update_batch<MuonEltArgs>(
        counts, nb, 1, kMuonEltTile,
        [&](MuonEltSeg &g, int b) {
            const kf_muon_apply &h = hyper[b];
            g = MuonEltSeg{params[b], xs[b], nullptr, counts[b],
                           static_cast<float>(1.0 - h.lr * h.weight_decay),
                           static_cast<float>(-h.lr * h.scale)};
        },
        [&](unsigned gx, unsigned gy, const MuonEltArgs &a) {
            muon_elt_kernel<true><<<dim3(gx, gy), kMuonBlock, 0, s>>>(a);
            return launch_status(fail_apply);
        });
}

int kf_muon_gemm_grouped(const kf_muon_gemm *problems, int count, KungFu_Datatype dt, float alpha,
                         float beta, void *stream)
{
    if (count < 0) return fail_gemm(KF_ERR_ARG, "KF_ERR_ARG", "count < 0");
    if (count == 0) return KF_OK;
    if (dt != KungFu_BFLOAT16) return fail_gemm(KF_ERR_DTYPE, "KF_ERR_DTYPE", "bf16 matrices only");
    if (!problems) return fail_gemm(KF_ERR_ARG, "KF_ERR_ARG", "null table");
    std::vector<size_t> tiles(count);
    for (int i = 0; i < count; ++i) {
        const kf_muon_gemm &q = problems[i];
        if (q.m < 1 || q.n < 1 || q.k < 1) {
            return fail_gemm(KF_ERR_ARG, "KF_ERR_ARG", "a zero or negative dimension");
        }
        if (q.k > INT_MAX - kMuonBK) {  // the K walk's last step stays an int
            return fail_gemm(KF_ERR_ARG, "KF_ERR_ARG", "k above INT_MAX - 32");
        }
        if (!q.a || !q.b || !q.c) return fail_gemm(KF_ERR_ARG, "KF_ERR_ARG", "null matrix");
        if (off(q.a, 2) || off(q.b, 2) || off(q.c, 2) || off(q.cin, 2)) {
            return fail_gemm(KF_ERR_ARG, "KF_ERR_ARG", "misaligned pointer");
        }
        if (q.trans_a < 0 || q.trans_a > 1 || q.trans_b < 0 || q.trans_b > 1) {
            return fail_gemm(KF_ERR_ARG, "KF_ERR_ARG", "trans_a and trans_b are 0 or 1");
        }
        // a stored matrix's row: op(A) is m x k, stored k x m when transposed
        if (q.lda < (q.trans_a ? q.m : q.k) || q.ldb < (q.trans_b ? q.k : q.n) || q.ldc < q.n ||
            (q.cin && q.ldcin < q.n)) {
            return fail_gemm(KF_ERR_ARG, "KF_ERR_ARG", "a leading dimension smaller than the row");
        }
        tiles[i] = static_cast<size_t>((q.m + kMuonTile - 1) / kMuonTile) *
                   static_cast<size_t>((q.n + kMuonTile - 1) / kMuonTile);
        if (tiles[i] > 0x400000u) {  // plan_update_batch's most blocks of one segment
            return fail_gemm(KF_ERR_ARG, "KF_ERR_ARG", "more than 2^22 tiles in one problem");
        }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    return plan_update_batch<MuonGemmArgs>(
        tiles.data(), count, 1, 1,
        [&](MuonGemmSeg &g, int i) {
            const kf_muon_gemm &q = problems[i];
            const int avec = !off(q.a, 16) && q.lda % 8 == 0, bvec = !off(q.b, 16) && q.ldb % 8 == 0;
            g = MuonGemmSeg{static_cast<const uint16_t *>(q.a), static_cast<const uint16_t *>(q.b),
                            static_cast<const uint16_t *>(q.cin), static_cast<uint16_t *>(q.c),
                            q.m, q.n, q.k, q.lda, q.ldb, q.cin ? q.ldcin : 0, q.ldc,
                            (q.trans_a ? 1 : 0) | (q.trans_b ? 2 : 0) | (avec ? 4 : 0) | (bvec ? 8 : 0)};
        },
        [&](unsigned gx, unsigned gy, const MuonGemmArgs &a) {
            muon_gemm_kernel<<<dim3(gx, gy), kMuonBlock, 0, s>>>(a, alpha, beta);
            return launch_status(fail_gemm);
        });
}

int kf_muon_syrk_grouped(const kf_muon_gemm *problems, int count, KungFu_Datatype dt, float alpha,
                         float beta, void *stream)
{
    if (count < 0) return fail_syrk(KF_ERR_ARG, "KF_ERR_ARG", "count < 0");
    if (count == 0) return KF_OK;
    if (dt != KungFu_BFLOAT16) return fail_syrk(KF_ERR_DTYPE, "KF_ERR_DTYPE", "bf16 matrices only");
    if (!problems) return fail_syrk(KF_ERR_ARG, "KF_ERR_ARG", "null table");
    std::vector<size_t> tiles(count);
    for (int i = 0; i < count; ++i) {
        const kf_muon_gemm &q = problems[i];
        if (q.m < 1 || q.k < 1) {
            return fail_syrk(KF_ERR_ARG, "KF_ERR_ARG", "a zero or negative dimension");
        }
        if (q.k > INT_MAX - kMuonBK) {
            return fail_syrk(KF_ERR_ARG, "KF_ERR_ARG", "k above INT_MAX - 32");
        }
        if (q.n != q.m || q.b) {
            return fail_syrk(KF_ERR_ARG, "KF_ERR_ARG",
                             "a symmetric product has n == m and no b (both operands are a)");
        }
        if (!q.a || !q.c) return fail_syrk(KF_ERR_ARG, "KF_ERR_ARG", "null matrix");
        if (off(q.a, 2) || off(q.c, 2) || off(q.cin, 2)) {
            return fail_syrk(KF_ERR_ARG, "KF_ERR_ARG", "misaligned pointer");
        }
        if (q.trans_a < 0 || q.trans_a > 1) {
            return fail_syrk(KF_ERR_ARG, "KF_ERR_ARG", "trans_a is 0 or 1");
        }
        if (q.lda < (q.trans_a ? q.m : q.k) || q.ldc < q.m || (q.cin && q.ldcin < q.m)) {
            return fail_syrk(KF_ERR_ARG, "KF_ERR_ARG", "a leading dimension smaller than the row");
        }
        const size_t tm = static_cast<size_t>((q.m + kMuonTile - 1) / kMuonTile);
        tiles[i]        = tm * (tm + 1) / 2;  // the lower triangle of the tile grid
        if (tiles[i] > 0x400000u) {
            return fail_syrk(KF_ERR_ARG, "KF_ERR_ARG", "more than 2^22 tiles in one problem");
        }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    return plan_update_batch<MuonGemmArgs>(
        tiles.data(), count, 1, 1,
        [&](MuonGemmSeg &g, int i) {
            const kf_muon_gemm &q = problems[i];
            const int avec = !off(q.a, 16) && q.lda % 8 == 0, cvec = !off(q.c, 16) && q.ldc % 8 == 0;
            g = MuonGemmSeg{static_cast<const uint16_t *>(q.a), nullptr,
                            static_cast<const uint16_t *>(q.cin), static_cast<uint16_t *>(q.c),
                            q.m, q.m, q.k, q.lda, 0, q.cin ? q.ldcin : 0, q.ldc,
                            (q.trans_a ? 1 : 0) | (avec ? 4 : 0) | (cvec ? 16 : 0)};
        },
        [&](unsigned gx, unsigned gy, const MuonGemmArgs &a) {
            muon_syrk_kernel<<<dim3(gx, gy), kMuonBlock, 0, s>>>(a, alpha, beta);
            return launch_status(fail_syrk);
        });
}

}  // extern "C"
