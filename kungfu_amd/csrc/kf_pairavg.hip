// kf_pairavg.hip — the device-side model store of PairAveragingOptimizer
// (AD-PSGD, async_sgd.py): every rank publishes whole snapshots of its
// variables into slots in its own HBM, and a peer pulls the latest one out of
// them over the pair's xGMI link and blends it into its own variables
// (include/kungfu_amd.h "pair averaging").
//
// Per rank:
//   slots    S snapshot slots in ONE device allocation (one IPC handle); a slot
//            holds every variable span at a 16-byte aligned offset;
//   control  uncached fine-grained device words (as kf_signal_alloc(.., 0)),
//            exported too: ctrl[0] = latest (versions published, 0 = none),
//            ctrl[1 + s] = lock[s], a seqlock that is odd while slot s is
//            being written;
//   private  a staging buffer of one slot, and state words: four counters
//            (valid, torn, empty, published) and the pick record.
//
// publish (version n = published + 1 -> slot n % S), three launches:
//   begin  lock[s] += 1 (odd), release at system scope
//   copy   variables -> slot s
//   end    lock[s] += 1 (even), latest = n, both release at system scope
// pull_average(target), four launches:
//   pick   v0 = latest, s = v0 % S, l0 = lock[s] (acquire, system scope)
//   fetch  the target's slot s -> staging
//   check  l1 = lock[s]; valid = (l1 == l0)
//   blend  valid: v = fl_T(0.5 * fl_T(v + staged)); else v untouched
// The launch boundaries order the markers and the data ("no in-launch
// ticket"). A reader validates AFTER it has read, which is why
// the snapshot goes through staging: an in-place blend would already have
// overwritten the variables when the check fails.
//
// No kernel here waits, spins or loops on a value another rank writes: a
// torn or empty pull is skipped and counted, never retried on the device.
//
// Memory visibility: slot data is ordinary (coarse-grained) device memory
// read by a peer. That leans on what the pull and push exchanges of
// kf_p2p.hip lean on: the writer's stores are released at its kernel end and
// the reader's kernel start invalidates non-local lines. Like them it has
// only ever run with the ranks as processes on ONE GPU; behaviour across two
// physical GPUs is unmeasured.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "kf_reduce_kernels.hpp"
#include "kungfu_amd.h"

namespace kf
{
#define KF_PA_GLOBAL __attribute__((address_space(1)))

typedef unsigned long long pa_u64;

// state words (private, ordinary device memory)
enum {
    PA_VALID = 0, PA_TORN = 1, PA_EMPTY = 2, PA_PUBLISHED = 3,  // counters
    PA_PICK_SLOT = 4, PA_PICK_LOCK0 = 5, PA_PICK_VERSION = 6,
    PA_PICK_STATE = 7,  // 0 = picked, 1 = empty, 2 = torn
    PA_PICK_VALID = 8,
    PA_WORDS = 16,
};

// Up to KF_MAX_SEGMENTS spans of one launch: the variable span, its byte
// offset inside a slot (and inside staging), its length in bytes.
struct PaSegs {
    char *v[KF_MAX_SEGMENTS];
    size_t off[KF_MAX_SEGMENTS];
    size_t len[KF_MAX_SEGMENTS];
};

constexpr int kPaBlock  = 256;
constexpr int kPaUnroll = 4;  // 16-B vectors per lane per tile

__device__ __forceinline__ pa_u64 ld_acq(const pa_u64 *p)
{
    return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ void st_rel(pa_u64 *p, pa_u64 v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// nvec 16-B vectors src -> dst, tiles `blk`, `blk + nblk`, ...: copy_kernel's
// shape (kf_p2p.hip), non-temporal both ways.
__device__ __forceinline__ void pa_copy_vecs(const KF_PA_GLOBAL u32x4 *src, KF_PA_GLOBAL u32x4 *dst,
                                             size_t nvec, size_t blk, size_t nblk)
{
    const size_t tile = kPaBlock * kPaUnroll;
    for (size_t t = blk; t * tile < nvec; t += nblk) {
        const size_t v0 = t * tile + threadIdx.x;
        u32x4 r[kPaUnroll];
#pragma unroll
        for (int u = 0; u < kPaUnroll; ++u) {
            if (v0 + u * kPaBlock < nvec) r[u] = __builtin_nontemporal_load(src + v0 + u * kPaBlock);
        }
#pragma unroll
        for (int u = 0; u < kPaUnroll; ++u) {
            if (v0 + u * kPaBlock < nvec) __builtin_nontemporal_store(r[u], dst + v0 + u * kPaBlock);
        }
    }
}

__global__ void pairavg_begin_kernel(pa_u64 *ctrl, const pa_u64 *st, unsigned S)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const pa_u64 n = st[PA_PUBLISHED] + 1;
    pa_u64 *lock   = ctrl + 1 + n % S;
    st_rel(lock, __hip_atomic_load(lock, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) + 1);
}

// variables -> slot (published + 1) % S. Block b serves span b % nseg; the
// bytes past a span's last whole vector (fewer than 16) go one per lane of
// the span's first block.
__global__ void __launch_bounds__(kPaBlock)
    pairavg_copy_kernel(PaSegs segs, int nseg, char *slots, size_t slot_bytes, const pa_u64 *st,
                        unsigned S)
{
    const int s       = static_cast<int>(blockIdx.x % nseg);
    const size_t slot = static_cast<size_t>((st[PA_PUBLISHED] + 1) % S);
    const KF_PA_GLOBAL char *src = (const KF_PA_GLOBAL char *)segs.v[s];
    KF_PA_GLOBAL char *dst       = (KF_PA_GLOBAL char *)(slots + slot * slot_bytes + segs.off[s]);
    const size_t len  = segs.len[s];
    const size_t nvec = len / 16;
    const size_t blk  = blockIdx.x / nseg;
    pa_copy_vecs(reinterpret_cast<const KF_PA_GLOBAL u32x4 *>(src),
                 reinterpret_cast<KF_PA_GLOBAL u32x4 *>(dst), nvec, blk, gridDim.x / nseg);
    const size_t i = nvec * 16 + threadIdx.x;
    if (blk == 0 && i < len) dst[i] = src[i];
}

__global__ void pairavg_end_kernel(pa_u64 *ctrl, pa_u64 *st, unsigned S)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const pa_u64 n = st[PA_PUBLISHED] + 1;
    pa_u64 *lock   = ctrl + 1 + n % S;
    st_rel(lock, __hip_atomic_load(lock, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) + 1);
    st_rel(ctrl, n);
    st[PA_PUBLISHED] = n;
}

__global__ void pairavg_pick_kernel(const pa_u64 *tctrl, pa_u64 *st, unsigned S)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const pa_u64 v0 = ld_acq(tctrl);
    const pa_u64 s  = v0 % S;
    const pa_u64 l0 = ld_acq(tctrl + 1 + s);
    st[PA_PICK_SLOT]    = s;
    st[PA_PICK_LOCK0]   = l0;
    st[PA_PICK_VERSION] = v0;
    st[PA_PICK_STATE]   = v0 == 0 ? 1 : ((l0 & 1) ? 2 : 0);
    st[PA_PICK_VALID]   = 0;
}

// The target's picked slot -> staging, as one flat range (a slot is a whole
// number of 16-B vectors). Every block reads the slot index from the local
// pick record, so the choice is uniform across the grid; an empty or torn
// pick copies nothing.
__global__ void __launch_bounds__(kPaBlock)
    pairavg_fetch_kernel(const char *tslots, size_t slot_bytes, char *staging, const pa_u64 *st)
{
    if (st[PA_PICK_STATE] != 0) return;
    const KF_PA_GLOBAL char *src =
        (const KF_PA_GLOBAL char *)(tslots + static_cast<size_t>(st[PA_PICK_SLOT]) * slot_bytes);
    pa_copy_vecs(reinterpret_cast<const KF_PA_GLOBAL u32x4 *>(src),
                 reinterpret_cast<KF_PA_GLOBAL u32x4 *>((KF_PA_GLOBAL char *)staging),
                 slot_bytes / 16, blockIdx.x, gridDim.x);
}

__global__ void pairavg_check_kernel(const pa_u64 *tctrl, pa_u64 *st)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const pa_u64 state = st[PA_PICK_STATE];
    pa_u64 valid       = 0;
    if (state == 1) {
        st[PA_EMPTY] += 1;
    } else if (state == 2) {
        st[PA_TORN] += 1;
    } else {
        const pa_u64 l1 = ld_acq(tctrl + 1 + st[PA_PICK_SLOT]);
        valid           = l1 == st[PA_PICK_LOCK0];
        st[valid ? PA_VALID : PA_TORN] += 1;
    }
    st[PA_PICK_VALID] = valid;
}

// fl_T(0.5 * fl_T(v + o)): TF's 0.5 * (v + other_v) in the tensor's dtype
// (async_sgd.py:130-133), every operation rounded to T, no contraction;
// f16 / bf16 compute in fp32 and round to T after the add and the multiply.
template <typename T> struct PairElt;
template <> struct PairElt<float> {
    using S = float;
    __device__ static S avg(S v, S o) { return __fmul_rn(0.5f, __fadd_rn(v, o)); }
};
template <> struct PairElt<double> {
    using S = double;
    __device__ static S avg(S v, S o) { return __dmul_rn(0.5, __dadd_rn(v, o)); }
};
template <> struct PairElt<f16_t> {
    using S = uint16_t;
    __device__ static S avg(S v, S o)
    {
        // widen, one operation, narrow: compiled to the native fp16 operation
        // (v_pk_add_f16, v_pk_mul_f16: the same correctly rounded value, and a
        // -0 product stays -0). f32_product_to_f16 would keep the multiply in
        // fp32 (16 packed operations -> 34 scalar ones); tests/test_isa.py
        // finds the x * y + 0 form if a compiler ever picks it here.
        const float s = f16_to_f32(f32_to_f16(__fadd_rn(f16_to_f32(v), f16_to_f32(o))));
        return f32_to_f16(__fmul_rn(0.5f, s));
    }
};
template <> struct PairElt<bf16_t> {
    using S = uint16_t;
    __device__ static S avg(S v, S o)
    {
        const float s = bf16_to_f32(f32_to_bf16(__fadd_rn(bf16_to_f32(v), bf16_to_f32(o))));
        return f32_to_bf16(__fmul_rn(0.5f, s));
    }
};

template <typename T> __device__ __forceinline__ u32x4 pair_vec(const u32x4 &rv, const u32x4 &ro)
{
    using S = typename PairElt<T>::S;
    Vec<S> v, o;
    __builtin_memcpy(&v, &rv, 16);
    __builtin_memcpy(&o, &ro, 16);
#pragma unroll
    for (int e = 0; e < Vec<S>::N; ++e) v.e[e] = PairElt<T>::avg(v.e[e], o.e[e]);
    u32x4 r;
    __builtin_memcpy(&r, &v, 16);
    return r;
}

// All spans of one launch. `valid` is one word of device memory, the same for
// every lane of the grid: no divergence, and without it no store at all.
template <typename T>
__global__ void __launch_bounds__(kPaBlock)
    pairavg_blend_kernel(PaSegs segs, int nseg, const char *staging, const pa_u64 *st)
{
    if (st[PA_PICK_VALID] == 0) return;
    using S           = typename PairElt<T>::S;
    const int s       = static_cast<int>(blockIdx.x % nseg);
    KF_PA_GLOBAL char *pv       = (KF_PA_GLOBAL char *)segs.v[s];
    const KF_PA_GLOBAL char *po = (const KF_PA_GLOBAL char *)(staging + segs.off[s]);
    KF_PA_GLOBAL u32x4 *vv       = reinterpret_cast<KF_PA_GLOBAL u32x4 *>(pv);
    const KF_PA_GLOBAL u32x4 *vo = reinterpret_cast<const KF_PA_GLOBAL u32x4 *>(po);
    const size_t len  = segs.len[s];
    const size_t nvec = len / 16;
    const size_t blk  = blockIdx.x / nseg;
    const size_t nblk = gridDim.x / nseg;
    const size_t tile = kPaBlock * kPaUnroll;
    for (size_t t = blk; t * tile < nvec; t += nblk) {
        const size_t v0 = t * tile + threadIdx.x;
        u32x4 rv[kPaUnroll], ro[kPaUnroll];
#pragma unroll
        for (int u = 0; u < kPaUnroll; ++u) {
            if (v0 + u * kPaBlock < nvec) {
                rv[u] = __builtin_nontemporal_load(vv + v0 + u * kPaBlock);
                ro[u] = __builtin_nontemporal_load(vo + v0 + u * kPaBlock);
            }
        }
#pragma unroll
        for (int u = 0; u < kPaUnroll; ++u) {
            if (v0 + u * kPaBlock < nvec) {
                __builtin_nontemporal_store(pair_vec<T>(rv[u], ro[u]), vv + v0 + u * kPaBlock);
            }
        }
    }
    // the elements past the last whole vector (fewer than 16 bytes of them)
    const size_t i = nvec * (16 / sizeof(S)) + threadIdx.x;
    if (blk == 0 && i < len / sizeof(S)) {
        KF_PA_GLOBAL S *ev       = reinterpret_cast<KF_PA_GLOBAL S *>(pv);
        const KF_PA_GLOBAL S *eo = reinterpret_cast<const KF_PA_GLOBAL S *>(po);
        ev[i]                    = PairElt<T>::avg(ev[i], eo[i]);
    }
}

}  // namespace kf

struct kf_pairavg {
    std::vector<char *> span;   // the local variable spans
    std::vector<size_t> off;    // each span's byte offset inside a slot
    std::vector<size_t> len;    // bytes
    size_t maxlen      = 0;
    size_t slot_bytes  = 0;     // a multiple of 16
    int slots          = 0;
    int world          = 0;
    int rank           = 0;
    KungFu_Datatype dt = KungFu_FLOAT;
    char *slot_mem     = nullptr;  // slots * slot_bytes
    char *staging      = nullptr;  // slot_bytes
    kf::pa_u64 *ctrl   = nullptr;  // 1 + slots uncached words
    kf::pa_u64 *st     = nullptr;  // PA_WORDS private words
    std::vector<const char *> peer_slots;      // [world], as mapped here
    std::vector<const kf::pa_u64 *> peer_ctrl;  // [world]
};

namespace
{
using namespace kf;

thread_local std::string t_pa_error;

int fail(int rc, const char *name, const std::string &what)
{
    t_pa_error = std::string(name) + ": " + what;
    return rc;
}

int arg_fail(const std::string &what) { return fail(KF_ERR_ARG, "KF_ERR_ARG", what); }

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

unsigned blocks_for(size_t bytes)
{
    const size_t tile = static_cast<size_t>(kPaBlock) * kPaUnroll * 16;
    size_t bx         = (bytes + tile - 1) / tile;
    if (bx > (size_t(1) << 16)) bx = size_t(1) << 16;
    return static_cast<unsigned>(bx < 1 ? 1 : bx);
}

// f(segs, nseg, blocks per span) for every group of up to KF_MAX_SEGMENTS spans
template <typename F> void for_span_groups(const kf_pairavg *p, F f)
{
    const int n = static_cast<int>(p->span.size());
    for (int i0 = 0; i0 < n; i0 += KF_MAX_SEGMENTS) {
        const int k = n - i0 < KF_MAX_SEGMENTS ? n - i0 : KF_MAX_SEGMENTS;
        PaSegs segs;
        size_t maxlen = 0;
        for (int i = 0; i < k; ++i) {
            segs.v[i]   = p->span[i0 + i];
            segs.off[i] = p->off[i0 + i];
            segs.len[i] = p->len[i0 + i];
            if (segs.len[i] > maxlen) maxlen = segs.len[i];
        }
        if (maxlen) f(segs, k, blocks_for(maxlen));
    }
}

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return KF_OK;
}

int need_target(const kf_pairavg *p, int target, const char *fn)
{
    if (!p) return arg_fail(std::string(fn) + ": null plan");
    if (target < 0 || target >= p->world) return arg_fail(std::string(fn) + ": target out of range");
    if (!p->peer_slots[target] || !p->peer_ctrl[target]) {
        return arg_fail(std::string(fn) + ": kf_pairavg_set_peers has not been called");
    }
    return KF_OK;
}

}  // namespace

extern "C" {

kf_pairavg_t *kf_pairavg_create(const void *const *spans, const size_t *span_bytes, int nspan,
                                KungFu_Datatype dt, int slots, int world, int rank)
{
    if (nspan <= 0 || !spans || !span_bytes) {
        arg_fail("kf_pairavg_create: at least one span, and non-null tables");
        return nullptr;
    }
    const int sz = elt_size(dt);
    if (sz == 0) {
        fail(KF_ERR_DTYPE, "KF_ERR_DTYPE", "kf_pairavg_create: f32, f16, bf16 and f64 only");
        return nullptr;
    }
    if (slots < 2 || slots > 64) {
        arg_fail("kf_pairavg_create: 2 to 64 slots");
        return nullptr;
    }
    if (world < 1 || rank < 0 || rank >= world) {
        arg_fail("kf_pairavg_create: rank must lie in [0, world)");
        return nullptr;
    }
    kf_pairavg *p = new kf_pairavg;
    size_t off    = 0;
    for (int i = 0; i < nspan; ++i) {
        const size_t n = span_bytes[i];
        if (n && !spans[i]) {
            arg_fail("kf_pairavg_create: null pointer in a non-empty span");
            delete p;
            return nullptr;
        }
        if (n && ((reinterpret_cast<uintptr_t>(spans[i]) % 16) || (n % sz))) {
            arg_fail("kf_pairavg_create: spans start 16-byte aligned and hold whole elements");
            delete p;
            return nullptr;
        }
        p->span.push_back(static_cast<char *>(const_cast<void *>(spans[i])));
        p->off.push_back(off);
        p->len.push_back(n);
        if (n > p->maxlen) p->maxlen = n;
        off += (n + 15) / 16 * 16;
    }
    p->slot_bytes = off ? off : 16;
    p->slots      = slots;
    p->world      = world;
    p->rank       = rank;
    p->dt         = dt;
    p->peer_slots.assign(world, nullptr);
    p->peer_ctrl.assign(world, nullptr);

    const size_t all = p->slot_bytes * static_cast<size_t>(slots);
    hipError_t e     = hipMalloc(reinterpret_cast<void **>(&p->slot_mem), all);
    if (e == hipSuccess) e = hipMemset(p->slot_mem, 0, all);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&p->staging), p->slot_bytes);
    if (e == hipSuccess) e = hipMemset(p->staging, 0, p->slot_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&p->st), PA_WORDS * sizeof(pa_u64));
    if (e == hipSuccess) e = hipMemset(p->st, 0, PA_WORDS * sizeof(pa_u64));
    if (e == hipSuccess) {
        // uncached fine-grained words, as kf_signal_alloc(.., host = 0)
        e = hipExtMallocWithFlags(reinterpret_cast<void **>(&p->ctrl),
                                  (1 + static_cast<size_t>(slots)) * sizeof(pa_u64),
                                  hipDeviceMallocUncached);
    }
    if (e == hipSuccess) e = hipMemset(p->ctrl, 0, (1 + static_cast<size_t>(slots)) * sizeof(pa_u64));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        hip_fail(e, "kf_pairavg_create");
        kf_pairavg_destroy(p);
        return nullptr;
    }
    p->peer_slots[rank] = p->slot_mem;
    p->peer_ctrl[rank]  = p->ctrl;
    return p;
}

int kf_pairavg_local(kf_pairavg_t *p, void **slot_base, void **ctrl_base, size_t *slot_bytes)
{
    if (!p) return arg_fail("kf_pairavg_local: null plan");
    if (slot_base) *slot_base = p->slot_mem;
    if (ctrl_base) *ctrl_base = p->ctrl;
    if (slot_bytes) *slot_bytes = p->slot_bytes;
    return KF_OK;
}

int kf_pairavg_set_peers(kf_pairavg_t *p, const void *const *slot_bases,
                         const void *const *ctrl_bases, int world)
{
    if (!slot_bases || !ctrl_bases || world < 1) {
        return arg_fail("kf_pairavg_set_peers: null table");
    }
    for (int r = 0; r < world; ++r) {
        if (!slot_bases[r] || (reinterpret_cast<uintptr_t>(slot_bases[r]) % 16)) {
            return arg_fail("kf_pairavg_set_peers: slot base must be non-null, 16-byte aligned");
        }
        if (!ctrl_bases[r] || (reinterpret_cast<uintptr_t>(ctrl_bases[r]) % 8)) {
            return arg_fail("kf_pairavg_set_peers: control base must be non-null, 8-byte aligned");
        }
    }
    if (!p) return arg_fail("kf_pairavg_set_peers: null plan");
    if (world != p->world) return arg_fail("kf_pairavg_set_peers: world differs from the plan's");
    for (int r = 0; r < world; ++r) {
        if (r == p->rank) continue;  // always this rank's own allocations
        p->peer_slots[r] = static_cast<const char *>(slot_bases[r]);
        p->peer_ctrl[r]  = static_cast<const pa_u64 *>(ctrl_bases[r]);
    }
    return KF_OK;
}

void kf_pairavg_destroy(kf_pairavg_t *p)
{
    if (!p) return;
    if (p->slot_mem) (void)hipFree(p->slot_mem);
    if (p->staging) (void)hipFree(p->staging);
    if (p->st) (void)hipFree(p->st);
    if (p->ctrl) (void)hipFree(p->ctrl);
    delete p;
}

int kf_pairavg_publish_begin(kf_pairavg_t *p, void *stream)
{
    if (!p) return arg_fail("kf_pairavg_publish_begin: null plan");
    pairavg_begin_kernel<<<1, 64, 0, static_cast<hipStream_t>(stream)>>>(
        p->ctrl, p->st, static_cast<unsigned>(p->slots));
    return launched("pairavg_begin_kernel launch");
}

int kf_pairavg_publish_copy(kf_pairavg_t *p, void *stream)
{
    if (!p) return arg_fail("kf_pairavg_publish_copy: null plan");
    hipStream_t s = static_cast<hipStream_t>(stream);
    for_span_groups(p, [&](const PaSegs &segs, int k, unsigned bx) {
        pairavg_copy_kernel<<<bx * k, kPaBlock, 0, s>>>(segs, k, p->slot_mem, p->slot_bytes, p->st,
                                                        static_cast<unsigned>(p->slots));
    });
    return launched("pairavg_copy_kernel launch");
}

int kf_pairavg_publish_end(kf_pairavg_t *p, void *stream)
{
    if (!p) return arg_fail("kf_pairavg_publish_end: null plan");
    pairavg_end_kernel<<<1, 64, 0, static_cast<hipStream_t>(stream)>>>(
        p->ctrl, p->st, static_cast<unsigned>(p->slots));
    return launched("pairavg_end_kernel launch");
}

int kf_pairavg_publish(kf_pairavg_t *p, void *stream)
{
    int rc = kf_pairavg_publish_begin(p, stream);
    if (rc == KF_OK) rc = kf_pairavg_publish_copy(p, stream);
    if (rc == KF_OK) rc = kf_pairavg_publish_end(p, stream);
    return rc;
}

int kf_pairavg_pick(kf_pairavg_t *p, int target, void *stream)
{
    const int rc = need_target(p, target, "kf_pairavg_pick");
    if (rc != KF_OK) return rc;
    pairavg_pick_kernel<<<1, 64, 0, static_cast<hipStream_t>(stream)>>>(
        p->peer_ctrl[target], p->st, static_cast<unsigned>(p->slots));
    return launched("pairavg_pick_kernel launch");
}

int kf_pairavg_fetch(kf_pairavg_t *p, int target, void *stream)
{
    const int rc = need_target(p, target, "kf_pairavg_fetch");
    if (rc != KF_OK) return rc;
    pairavg_fetch_kernel<<<blocks_for(p->slot_bytes), kPaBlock, 0, static_cast<hipStream_t>(stream)>>>(
        p->peer_slots[target], p->slot_bytes, p->staging, p->st);
    return launched("pairavg_fetch_kernel launch");
}

int kf_pairavg_check(kf_pairavg_t *p, int target, void *stream)
{
    const int rc = need_target(p, target, "kf_pairavg_check");
    if (rc != KF_OK) return rc;
    pairavg_check_kernel<<<1, 64, 0, static_cast<hipStream_t>(stream)>>>(p->peer_ctrl[target],
                                                                         p->st);
    return launched("pairavg_check_kernel launch");
}

int kf_pairavg_blend(kf_pairavg_t *p, void *stream)
{
    if (!p) return arg_fail("kf_pairavg_blend: null plan");
    hipStream_t s = static_cast<hipStream_t>(stream);
    for_span_groups(p, [&](const PaSegs &segs, int k, unsigned bx) {
        const unsigned grid = bx * k;
        switch (p->dt) {
        case KungFu_FLOAT:
            pairavg_blend_kernel<float><<<grid, kPaBlock, 0, s>>>(segs, k, p->staging, p->st);
            break;
        case KungFu_DOUBLE:
            pairavg_blend_kernel<double><<<grid, kPaBlock, 0, s>>>(segs, k, p->staging, p->st);
            break;
        case KungFu_FLOAT16:
            pairavg_blend_kernel<f16_t><<<grid, kPaBlock, 0, s>>>(segs, k, p->staging, p->st);
            break;
        default:
            pairavg_blend_kernel<bf16_t><<<grid, kPaBlock, 0, s>>>(segs, k, p->staging, p->st);
            break;
        }
    });
    return launched("pairavg_blend_kernel launch");
}

int kf_pairavg_pull_average(kf_pairavg_t *p, int target, void *stream)
{
    int rc = kf_pairavg_pick(p, target, stream);
    if (rc == KF_OK) rc = kf_pairavg_fetch(p, target, stream);
    if (rc == KF_OK) rc = kf_pairavg_check(p, target, stream);
    if (rc == KF_OK) rc = kf_pairavg_blend(p, stream);
    return rc;
}

int kf_pairavg_counters(kf_pairavg_t *p, uint64_t *out, void *stream)
{
    if (!p || !out) return arg_fail("kf_pairavg_counters: null plan or out");
    const hipError_t e = hipMemcpyAsync(out, p->st, 4 * sizeof(uint64_t), hipMemcpyDefault,
                                        static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "kf_pairavg_counters");
    return KF_OK;
}

const char *kf_pairavg_last_error(void) { return t_pa_error.c_str(); }

}  // extern "C"
