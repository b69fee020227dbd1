// kf_update_batch.hpp — the launch machinery the batched optimizer-update
// kernels share (kf_sgd.hip, kf_adam.hip, kf_adam_master.hip, kf_adam_sr.hip,
// kf_adam8.hip, kf_lamb.hip; kf_step_gate.hip takes the failure reporter): the
// host's launch planner, the device's segment lookup and /np dispatch, and the
// entry points' validation ladder. The arithmetic is shared in kf_sgd_elt.hpp,
// kf_adam_math.hpp and kf_lamb_math.hpp; the tile loops are each kernel's own
// (DESIGN.md §13, §21).
//
// A kernarg struct ARGS has `seg[NSEG]` (one entry per segment, the kernel's
// own type), `unsigned blk0[NSEG + 1]` and `int nseg`. Segments of about equal
// size are the rows of a 2-D grid, others share a 1-D grid through the search
// table blk0.
//
// The host part is plain C++17; what needs HIP is under __HIPCC__.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <type_traits>

#include "kungfu_amd.h"

namespace kf
{
void set_last_error(const std::string &msg);  // kf_capi.hip: kf_last_error's text

// An entry point's failure: kf_last_error's text is "<code's name>: <entry
// point>: <what>".
struct UpdateFail {
    const char *entry;
    int operator()(int rc, const char *name, const std::string &what) const
    {
        set_last_error(std::string(name) + ": " + entry + ": " + what);
        return rc;
    }
};

inline bool off16(const void *p) { return (reinterpret_cast<uintptr_t>(p) % 16) != 0; }

// One pointer table of an Adam-family update call: a pointer per segment, what
// a non-empty segment's pointer must be a multiple of (a power of two), and the
// refusal's text where it is not. ptr == nullptr with `absent`: the entry has
// no such table.
struct UpdateTab {
    const void *const *ptr;
    unsigned align;
    const char *misaligned;
    bool absent = false;
};
constexpr const char *kOff16 = "pointers must be 16-byte aligned";

// A gated call's gate and step state, and, once the checks have run, its one
// hyper: the caller's with both bias corrections 1 (they are the device's).
struct UpdateGate {
    const kf_step_gate *gate;
    const kf_step_state *state;
    kf_adam_hyper one;
};

inline int no_check(int) { return KF_OK; }

// The checks every Adam-family entry makes before its first HIP call, in the
// one order they all keep: nb < 0, nb == 0 (KF_OK: the caller returns on
// nb == 0 too), a gated call's gate and state, the tables (`also`: further
// arrays of the entry's own that must not be null), np, and per non-empty
// segment first(b), null pointers, alignment in table order, the bias
// corrections, last(b). dtype() is the entry's own check with its own
// text; it comes after the tables' check, or before it with dtype_first
// (LAMB). Afterwards `hyper` is what the kernels take: with a gate, g->one for
// every segment, else hyper[b].
template <size_t N, typename DTYPE, typename FIRST, typename LAST>
int check_update_batch(const UpdateFail &fail, const UpdateTab (&tabs)[N],
                       std::initializer_list<const void *> also, const size_t *counts, int nb,
                       int np, const kf_adam_hyper *&hyper, UpdateGate *g, bool dtype_first,
                       DTYPE &&dtype, FIRST &&first, LAST &&last)
{
    if (nb < 0) return fail(KF_ERR_ARG, "KF_ERR_ARG", "nb < 0");
    if (nb == 0) return KF_OK;
    if (g && (!g->gate || !g->state)) {
        return fail(KF_ERR_ARG, "KF_ERR_ARG", "null gate or step state");
    }
    int rc = dtype_first ? dtype() : KF_OK;
    if (rc != KF_OK) return rc;
    // the tables that are there, once: the segment loop does not look at `absent`
    const void *const *ptr[N];
    uintptr_t mask[N];
    size_t n   = 0;
    bool null = !counts || !hyper;
    for (const UpdateTab &t : tabs) {
        null = null || (!t.absent && !t.ptr);
        if (!t.ptr) continue;
        ptr[n]    = t.ptr;
        mask[n++] = t.align - 1;
    }
    for (const void *p : also) null = null || !p;
    if (null) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null table");
    rc = dtype_first ? KF_OK : dtype();
    if (rc != KF_OK) return rc;
    if (np < 0) return fail(KF_ERR_ARG, "KF_ERR_ARG", "np < 0");
    if (g) {
        g->one                  = *hyper;
        g->one.bias_correction1 = g->one.bias_correction2 = 1.0;
        hyper                   = &g->one;
    }
    for (int b = 0; b < nb; ++b) {
        if (counts[b] == 0) continue;
        if ((rc = first(b)) != KF_OK) return rc;
        bool none     = false;  // one pass: a null pointer, and the pointers' stray low bits
        uintptr_t off = 0;
        for (size_t i = 0; i < n; ++i) {
            const uintptr_t p = reinterpret_cast<uintptr_t>(ptr[i][b]);
            none              = none || p == 0;
            off |= p & mask[i];
        }
        if (none) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null pointer in a non-empty segment");
        if (off != 0) {  // the first misaligned table's text, in table order
            for (const UpdateTab &t : tabs) {
                if (t.ptr && (reinterpret_cast<uintptr_t>(t.ptr[b]) & (t.align - 1)) != 0) {
                    return fail(KF_ERR_ARG, "KF_ERR_ARG", t.misaligned);
                }
            }
        }
        const kf_adam_hyper &h = hyper[g ? 0 : b];
        if (!(h.bias_correction1 > 0) || !(h.bias_correction2 > 0)) {
            return fail(KF_ERR_ARG, "KF_ERR_ARG", "bias corrections must be > 0");
        }
        if ((rc = last(b)) != KF_OK) return rc;
    }
    return KF_OK;
}

// The launches of one update call over counts[0..nb): every non-empty segment
// takes the next entry of an ARGS, filled by fill(a.seg[i], b), and
// launch(grid_x, grid_y, a) -> status is called for every full table, before a
// grid would grow too large, and at the end. A unit is `elts` elements (what
// one lane loads at once), a tile `tile` units (what one block does per
// round). The first status that is not KF_OK is returned, and nothing is
// launched after it.
template <typename ARGS, typename FILL, typename LAUNCH>
int plan_update_batch(const size_t *counts, int nb, size_t elts, size_t tile, FILL &&fill,
                      LAUNCH &&launch)
{
    constexpr int NSEG = std::extent<decltype(ARGS::seg)>::value;
    static_assert(std::extent<decltype(ARGS::blk0)>::value == NSEG + 1, "blk0 closes the table");
    ARGS a;
    a.nseg        = 0;
    size_t blocks = 0, widest = 0;
    auto flush    = [&]() -> int {
        if (a.nseg == 0) return KF_OK;
        a.blk0[a.nseg] = static_cast<unsigned>(blocks);
        // one row per segment when that at most doubles the grid
        const bool rows = a.nseg > 1 && widest * a.nseg <= 2 * blocks;
        const int rc    = rows ? launch(static_cast<unsigned>(widest), static_cast<unsigned>(a.nseg), a)
                               : launch(static_cast<unsigned>(blocks), 1u, a);
        a.nseg = 0;
        blocks = widest = 0;
        return rc;
    };
    for (int b = 0; b < nb; ++b) {
        const size_t n = counts[b];
        if (n == 0) continue;
        size_t nblk = (n / elts + tile - 1) / tile;  // one block per tile
        if (nblk < 1) nblk = 1;                      // a tail alone
        if (nblk > 0x400000u) nblk = 0x400000u;      // then blocks stride over the tiles
        if (blocks + nblk > 0x7fffffu) {             // grid * block stays below 2^32 threads,
            const int rc = flush();                  // also as rows (at most twice the blocks)
            if (rc != KF_OK) return rc;
        }
        fill(a.seg[a.nseg], b);
        a.blk0[a.nseg] = static_cast<unsigned>(blocks);
        blocks += nblk;
        if (nblk > widest) widest = nblk;
        if (++a.nseg == NSEG) {
            const int rc = flush();
            if (rc != KF_OK) return rc;
        }
    }
    return flush();
}

#ifdef __HIPCC__
// The status of the launch just made.
inline int launch_status(const UpdateFail &fail)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return KF_OK;
    return fail(KF_ERR_HIP, "KF_ERR_HIP", std::string("launch: ") + hipGetErrorString(e));
}

// The segment of this block, and the block's place `blk` of `nblk` on it.
// Segments of about equal size (an exchange's shards of equal buckets) come
// as a 2-D grid, one row per segment: the segment is blockIdx.y, known before
// any kernarg load, and a row's blocks past the segment's last tile have
// nothing to do. Otherwise the segment of block b is the last s with
// blk0[s] <= b, searched in the kernarg table (wave-uniform scalar loads, one
// dependent load per step).
template <typename ARGS>
__device__ __forceinline__ int batch_segment(const ARGS &a, size_t &blk, size_t &nblk)
{
    const bool rows = gridDim.y > 1;
    int s           = static_cast<int>(blockIdx.y);
    blk             = blockIdx.x;
    nblk            = gridDim.x;
    if (!rows) {
        const unsigned b = blockIdx.x;
        int lo = 0, hi = a.nseg - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (b >= a.blk0[mid]) lo = mid;
            else hi = mid - 1;
        }
        s    = lo;
        blk  = b - a.blk0[s];
        nblk = a.blk0[s + 1] - a.blk0[s];
    }
    return s;
}

// The /np choice made once per kernel (kf_reduce_kernels.hpp EPI_MUL):
// f(std::integral_constant<int, DIV>).
template <typename F> __device__ __forceinline__ void dispatch_div(int div, F &&f)
{
    if (div == 0) f(std::integral_constant<int, 0>{});
    else if (div == 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 2>{});
}
#endif  // __HIPCC__

}  // namespace kf
