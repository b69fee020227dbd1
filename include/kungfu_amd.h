/*
 * kungfu_amd.h — C-ABI of the MI355X gradient-bucket reduce.
 *
 * Two layers live behind this header (libkungfu_amd.so, built from
 * kungfu_amd/csrc/ for gfx950):
 *
 *  B1  drop-in element kernel. Link-compatible with KungFu's base package:
 *        std_transform_2   replaces /root/reference/srcs/go/kungfu/base/op.cpp:57-93
 *                          (declared in srcs/cpp/include/kungfu/op.h:17-19)
 *        kungfu_type_size  replaces srcs/go/kungfu/base/dtype.c:7-35
 *                          (declared in srcs/cpp/include/kungfu/dtype.h:46)
 *        float16_sum       replaces srcs/go/kungfu/base/f16.c:25-50
 *                          (declared in srcs/go/kungfu/base/f16.h:7)
 *      These take HOST pointers, run the reduce on the GPU (pageable host
 *      memory -> HBM -> HIP kernel -> host) and return only when the output
 *      is written, as cgo requires (srcs/go/kungfu/base/op.go:27-35). Bad
 *      dtype/op -> exit(1), exactly like op.cpp:41,52,89 and dtype.c:31-33.
 *
 *  B2  bucket-level device API (the real fast path). Device
 *      pointers, a hipStream_t passed as void*, no allocation, no host sync,
 *      error codes instead of exit(). Safe to capture into a hipGraph.
 *
 * Enum values are bit-identical to the reference ABI:
 *      KungFu_Datatype  srcs/cpp/include/kungfu/dtype.h:21-39  ((cat<<16)|(bytes<<8)|8)
 *      KungFu_Op        srcs/cpp/include/kungfu/op.h:8-13
 * KungFu_BFLOAT16 is an extension (category 2, 2 bytes, bits-per-byte field 9
 * so it cannot collide with FLOAT16); the reference has no bf16 type and maps
 * TF bf16 onto FLOAT16 (srcs/cpp/include/kungfu/tensorflow/ops.h:21-22).
 */
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: exactly what this header
 * declares is exported. */
#pragma GCC visibility push(default)

/* ---- reference-compatible enums ---------------------------------------- */

enum KungFu_Datatype {
    KungFu_UINT8   = 0x00108,
    KungFu_UINT16  = 0x00208,
    KungFu_UINT32  = 0x00408,
    KungFu_UINT64  = 0x00808,
    KungFu_INT8    = 0x10108,
    KungFu_INT16   = 0x10208,
    KungFu_INT32   = 0x10408,
    KungFu_INT64   = 0x10808,
    KungFu_FLOAT16 = 0x20208,
    KungFu_FLOAT   = 0x20408,
    KungFu_DOUBLE  = 0x20808,
    KungFu_BOOL    = 0x30108,
    /* extension, not in the reference */
    KungFu_BFLOAT16 = 0x20209,
};
typedef enum KungFu_Datatype KungFu_Datatype;

enum KungFu_Op {
    KungFu_SUM  = 0,
    KungFu_MIN  = 1,
    KungFu_MAX  = 2,
    KungFu_PROD = 3,
};
typedef enum KungFu_Op KungFu_Op;

/* srcs/cpp/include/kungfu/strategy.h:7-17 */
enum KungFu_Strategy {
    KungFu_Tree                = 0,
    KungFu_BinaryTree          = 1,
    KungFu_Ring                = 2,
    KungFu_Star                = 3,
    KungFu_MultiStar           = 4,
    KungFu_Clique              = 5,
    KungFu_BinaryTreeStar      = 6,
    KungFu_MultiBinaryTreeStar = 7,
    KungFu_AUTO                = 8,
};
typedef enum KungFu_Strategy KungFu_Strategy;

/* ---- B1: drop-in host-pointer entry points ------------------------------ */

/* out[i] = o(input1[i], input2[i]) for i < n. out may alias input1 or input2
 * exactly. Replaces srcs/go/kungfu/base/op.cpp:57-93. */
void std_transform_2(const void *input1, const void *input2, void *output,
                     const int n, const KungFu_Datatype dt, const KungFu_Op o);

/* sizeof one element; unknown dtype -> message + exit(1).
 * Replaces srcs/go/kungfu/base/dtype.c:7-35. */
uint32_t kungfu_type_size(KungFu_Datatype dt);

/* z[i] = fp16(fp32(x[i]) + fp32(y[i])), round-to-nearest-even.
 * Replaces srcs/go/kungfu/base/f16.c:25-50. */
void float16_sum(void *z, const void *x, const void *y, int len);

/* ---- B2: bucket-level device API ---------------------------------------- */

enum KF_Status {
    KF_OK              = 0,
    KF_ERR_DTYPE       = 1, /* unsupported dtype                      */
    KF_ERR_OP          = 2, /* unsupported op for this dtype          */
    KF_ERR_ARG         = 3, /* null pointer with n>0, k out of range  */
    KF_ERR_HIP         = 4, /* a HIP runtime call failed              */
    KF_ERR_NO_DEVICE   = 5, /* no usable gfx950 device                */
    KF_ERR_IO          = 6, /* socket read/write failed               */
    KF_ERR_PROTO       = 7, /* rchannel framing/length/token mismatch  */
    KF_ERR_TIMEOUT     = 8, /* a device-side peer barrier gave up      */
    KF_ERR_RCCL        = 9, /* librccl missing or an RCCL call failed  */
};

/* Largest k accepted by kf_bucket_reduce*. */
#define KF_MAX_INPUTS 16

/* out[i] = (((in[0][i] o in[1][i]) o in[2][i]) ... o in[k-1][i])
 * Left fold in the given order: pass the peers in the reference's arrival or
 * ring order to reproduce its accumulation order bit for bit
 * (session.go:255-264 applies Transform2(recv, acc, peer) per hop).
 * fp16 rounds to fp16 after every hop, as the reference chain does; bf16
 * accumulates in fp32 and rounds once (build-defined, parity unpinned).
 * k == 1 is a copy. out may alias any input exactly. */
int kf_bucket_reduce(const void *const *inputs, int k, void *out, size_t n,
                     KungFu_Datatype dt, KungFu_Op op, void *stream);

/* S-SGD epilogue fused into the reduce: out[i] = fold_SUM(in[*][i]) / np,
 * a true IEEE division (TF's g / np, sync_sgd.py:103-104), so it is bit-exact
 * against "reduce, then divide" for every np. float types only. */
int kf_bucket_reduce_avg(const void *const *inputs, int k, void *out, size_t n,
                         KungFu_Datatype dt, int np, void *stream);

/* In-place scale of an already-summed shard: x[i] = x[i] / np (the step
 * between RCCL reduce-scatter and all-gather). float types only. */
int kf_bucket_div(void *x, size_t n, KungFu_Datatype dt, int np, void *stream);

/* Many independent buckets in one launch per 16 of them: bucket b is
 *   outs[b][i] = fold(inputs[b*k + 0][i], ..., inputs[b*k + k-1][i]), i < counts[b]
 * with the same arithmetic as kf_bucket_reduce (np == 0) or
 * kf_bucket_reduce_avg (np > 0: SUM then / np, float types). A bucket whose
 * pointers do not share one 16-B residue, and MIN / MAX / PROD, get a launch
 * each; k == 1 with np == 0 is a copy per bucket. For the per-bucket steps of
 * an exchange (every shard's /np, every bucket's fold of the received shards),
 * where one launch per 4 MiB bucket costs more than the bucket's HBM time. */
int kf_bucket_reduce_batch(const void *const *inputs, int k, void *const *outs,
                           const size_t *counts, int nb, KungFu_Datatype dt, KungFu_Op op,
                           int np, void *stream);

/* SMA epilogue (sma_sgd.py:60-65):
 *   v[i] = fl(fl(c1 * v[i]) + fl(c2 * fl(sum[i] / np)))
 * with c1 = (float)(1 - alpha), c2 = (float)alpha computed in double first,
 * as TF converts the Python constants. No FMA contraction. float types only. */
int kf_sma_blend(void *v, const void *sum, size_t n, KungFu_Datatype dt,
                 int np, double alpha, void *stream);
/* kf_sma_blend over nb buckets (vs[b] blended with sums[b], counts[b]
 * elements each, the same dtype, np and alpha) in one launch per 16 buckets;
 * the same bits as nb kf_sma_blend calls. */
int kf_sma_blend_batch(void *const *vs, const void *const *sums, const size_t *counts, int nb,
                       KungFu_Datatype dt, int np, double alpha, void *stream);

/* SGD update of nb segments of one float dtype in one launch per 32 of them
 * (kungfu_amd/csrc/kf_sgd.hip): torch.optim.SGD's single-tensor arithmetic on
 * a summed gradient, one IEEE operation per step, no contraction:
 *   g = np > 0 ? grads[b][i] / np : grads[b][i]     (kf_bucket_div's rounding)
 *   if weight_decay != 0:  g = g + weight_decay * p
 *   if momentum != 0:      m = first ? g : (momentum * m) + (c * g)
 *                          g = nesterov ? g + momentum * m : m
 *   p = p + nlr * g
 * with c = 1 - dampening and nlr = -lr computed in double, and every scalar
 * cast once to the compute type. f32 / f64 round every product and every sum
 * in that type. f16 / bf16 compute in fp32 and round to the storage type
 * after the /np, the weight-decay add, momentum * m, the momentum add, the
 * nesterov add and the final add (where torch's tensor ops do); the
 * alpha * x product and the add inside each are two fp32 roundings.
 * Segment b is counts[b] elements at params[b], grads[b] (read only) and
 * moms[b] with its own hyper[b] (a host array of nb, read before the call
 * returns). moms, or moms[b], may be NULL where momentum == 0: no momentum
 * stream; on a `first` step m is written and not read. Every pointer is
 * 16-byte aligned. g, p and m are read once, p and m written once. */
typedef struct { double lr, momentum, dampening, weight_decay; int nesterov; int first; } kf_sgd_hyper;
int kf_sgd_update_batch(void *const *params, const void *const *grads, void *const *moms,
                        const size_t *counts, int nb, KungFu_Datatype dt, int np,
                        const kf_sgd_hyper *hyper, void *stream);

/* Adam / AdamW update of nb segments of one dtype in one launch per 24 of
 * them (kungfu_amd/csrc/kf_adam.hip): torch.optim.Adam / AdamW's single-tensor
 * arithmetic on a summed gradient. Each parenthesised operation is one IEEE
 * operation, no contraction:
 *   g = np > 0 ? grads[b][i] / np : grads[b][i]     (kf_bucket_div's rounding)
 *   weight_decay != 0, decoupled == 0 (Adam, L2):  g = g + (wd*p)
 *   weight_decay != 0, decoupled != 0 (AdamW):     p = dk*p        dk = 1 - lr*wd
 *   m = (b1*m) + (c1*g)                          c1 = 1 - beta1
 *   v = (b2*v) + (c2*(g*g))                      c2 = 1 - beta2
 *   d = (sqrt(v) / s2) + eps                     s2 = sqrt(bias_correction2)
 *   p = p + (nss*(m / d))                        nss = -(lr / bias_correction1)
 * dk, c1, c2, s2 and nss are computed in double on the host and cast once to
 * the compute type. The caller passes the bias corrections 1 - beta^t of its
 * step t >= 1, computed in double (both must be > 0). The sqrt and both
 * divisions are correctly rounded. f32 / f64 round every operation in that
 * type. bf16 computes in fp32 and rounds to bf16 where torch's tensor ops
 * do: after the /np, after the L2 add or the decay multiply, after m (once:
 * torch's lerp_ is one op), after b2*v, after the v add, after the sqrt,
 * after the / s2, after the + eps and after the final add. m is two products
 * and a sum, not torch's lerp.
 * f32, f64 and bf16 only; the state (exp_avgs, exp_avg_sqs) has the
 * parameters' dtype and starts as zeros. f16 is KF_ERR_DTYPE: eps = 1e-8
 * rounds to 0 in f16, so every element with v == 0 would be 0 / 0.
 * Segment b is counts[b] elements at params[b], grads[b] (read only),
 * exp_avgs[b] and exp_avg_sqs[b] with its own hyper[b] (a host array of nb,
 * read before the call returns). Every pointer is 16-byte aligned. g, p, m
 * and v are read once, p, m and v written once. */
typedef struct { double lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2; int decoupled; } kf_adam_hyper;
int kf_adam_update_batch(void *const *params, const void *const *grads, void *const *exp_avgs,
                         void *const *exp_avg_sqs, const size_t *counts, int nb,
                         KungFu_Datatype dt, int np, const kf_adam_hyper *hyper, void *stream);

/* kf_adam_update_batch for 16-bit parameters with an fp32 master copy and
 * fp32 state (kungfu_amd/csrc/kf_adam_master.hip, one launch per 32 segments).
 * dt is the storage type of params16 / grads16, KungFu_BFLOAT16 or
 * KungFu_FLOAT16 (anything else is KF_ERR_DTYPE); masters, exp_avgs and
 * exp_avg_sqs are fp32. Per element:
 *   g = widen(grads16[b][i])                       (exact)
 *   (master, m, v) = kf_adam_update_batch's f32 arithmetic above, operation
 *                    for operation, on (master, g, m, v); the /np is the fp32
 *                    one and is not rounded to 16 bits
 *   params16[b][i] = narrow(master)                (round-to-nearest-even)
 * There is no other rounding to 16 bits anywhere, and the old value of
 * params16 is never read: the caller keeps params16 == narrow(masters). eps
 * stays fp32, so f16 parameters are taken; their gradients must be finite
 * (loss scaling and step skipping are kf_adam_master_update_batch_gated's,
 * below). Segment b is counts[b] elements with its own
 * hyper[b]; every pointer is 16-byte aligned. g (2 bytes), master, m and v
 * are read once; master, m, v and params16 (2 bytes) written once: 28 bytes
 * per element. */
int kf_adam_master_update_batch(void *const *params16, const void *const *grads16,
                                void *const *masters, void *const *exp_avgs,
                                void *const *exp_avg_sqs, const size_t *counts, int nb,
                                KungFu_Datatype dt, int np, const kf_adam_hyper *hyper,
                                void *stream);

/* ---- the gated step: one device-side verdict per optimizer step ----------
 *
 * Gradient-norm clipping, loss scaling and the skipping of a step whose
 * gradients are not finite need one global verdict between the reduce and the
 * update. It is computed on the device (kungfu_amd/csrc/kf_step_gate.hip) and
 * the gated update kernels read it from device memory, so the host never waits
 * for it.
 *
 * The device state is two plain structs. A gate serves one optimizer; a step
 * state serves one parameter group. Both start zero-filled, with loss_scale =
 * the initial scale (1 without loss scaling) and beta1_pow = beta2_pow = 1. */
typedef struct {
    int32_t skip;       /* this step's verdict: 1 = the gradients are not finite   */
    float grad_mul;     /* what the update multiplies g by: (float)(clip / scale)  */
    float loss_scale;   /* fp32; after a call, the scale the NEXT loss is given    */
    int32_t good_steps; /* applied steps since the scale last changed              */
    double grad_norm;   /* this step's norm of the unscaled, averaged gradient     */
    double total;       /* the sum of squares it came from (scaled gradients)      */
    uint64_t applied;   /* steps applied so far                                    */
    uint64_t skipped;   /* steps skipped so far                                    */
} kf_step_gate;
typedef struct {
    double beta1_pow;   /* beta1^step and beta2^step as running products in double */
    double beta2_pow;
    int64_t step;       /* applied steps of this group                             */
    double s2_f64;      /* sqrt(1 - beta2_pow), what the f64 kernel reads          */
    double nss_f64;     /* -(lr / (1 - beta1_pow))                                 */
    float s2;           /* the same two cast once to fp32: every other kernel      */
    float nss;
} kf_step_state;
typedef struct { double lr, beta1, beta2; } kf_step_group;

/* One verdict. sq is a device array of world * nplan doubles, sq[r * nplan +
 * k] the sum of squares of rank r's shards of plan k (kf_segnorm_run's total);
 * np[k] (host) is what plan k's gradients are still to be divided by: 0 when
 * they already hold the average. groups[j] (host) and states[j] (device,
 * contiguous) are parameter group j's. fp64 on one lane, one IEEE operation
 * per parenthesis, correctly rounded sqrt and divisions, no atomics:
 *   total = 0; for k in plan order:
 *       s = 0; for r in rank order: s = s + sq[r][k]
 *       if np[k] > 0: s = s / (np[k] * np[k])
 *       total = total + s
 *   skip      = !isfinite(total)
 *   grad_norm = sqrt(total) / loss_scale
 *   clip      = max_norm > 0 ? (x = max_norm / (grad_norm + 1e-6); x < 1 ? x : 1) : 1
 *   grad_mul  = (float)(clip / loss_scale)
 * with the loss_scale from before this call, the one the loss was multiplied
 * by. A non-finite total means a non-finite gradient element somewhere (f64
 * gradients whose squares overflow count as that). Then the loss scale, in
 * fp32, by torch.amp.GradScaler's rule:
 *   skip:  loss_scale = loss_scale * (float)backoff_factor; good_steps = 0
 *   else:  ++good_steps == growth_interval: loss_scale = loss_scale *
 *          (float)growth_factor unless that is not finite; good_steps = 0
 *          (growth_interval 0: the scale never grows)
 * and, only when !skip, every group:
 *   beta1_pow = beta1_pow * beta1; beta2_pow = beta2_pow * beta2; ++step
 *   s2_f64 = sqrt(1 - beta2_pow); nss_f64 = -(lr / (1 - beta1_pow))
 *   s2 = (float)s2_f64; nss = (float)nss_f64
 * A skipped step leaves every group's state as it was. The bias corrections
 * are running products in double, not beta^step: the host does not know which
 * steps were skipped. This is the gated path's own contract; after t applied
 * steps the product may differ from pow(beta, t) in its last places.
 * Any nplan >= 1, world >= 1 and ngroup >= 0: one launch for up to 64 plans
 * and 16 groups, more launches on the same stream beyond. Only queues
 * launches: no allocation, no host sync. max_norm <= 0 means no clipping. */
int kf_step_gate_update(const double *sq, int world, int nplan, const int *np,
                        const kf_step_group *groups, kf_step_state *states, int ngroup,
                        double max_norm, double growth_factor, double backoff_factor,
                        int growth_interval, kf_step_gate *gate, void *stream);

/* kf_adam_update_batch / kf_adam_master_update_batch under a gate (kernels of
 * their own beside the parents', kf_adam.hip / kf_adam_master.hip). They take
 * what their parents take, except: ONE hyper for the whole call, whose
 * bias_correction1 / bias_correction2 are ignored, and device pointers to the
 * gate and to the segments' group's step state, both written by an earlier
 * kf_step_gate_update on the same stream. Every block reads gate->skip; when
 * it is set the kernel returns without touching params, params16, masters,
 * exp_avgs or exp_avg_sqs. Otherwise s2 and nss come from *state (s2_f64 /
 * nss_f64 for f64) in place of the parent's kernarg scalars, and exactly one
 * operation joins the parent's sequence, directly after the /np:
 *   g = rnd(g * grad_mul)
 * rounded like every other operation there: to bf16 without master weights,
 * to fp32 on the master path, to the type itself for f32 / f64. Everything
 * else is the parent's arithmetic, operation for operation. */
int kf_adam_update_batch_gated(void *const *params, const void *const *grads,
                               void *const *exp_avgs, void *const *exp_avg_sqs,
                               const size_t *counts, int nb, KungFu_Datatype dt, int np,
                               const kf_adam_hyper *hyper, const kf_step_gate *gate,
                               const kf_step_state *state, void *stream);
int kf_adam_master_update_batch_gated(void *const *params16, const void *const *grads16,
                                      void *const *masters, void *const *exp_avgs,
                                      void *const *exp_avg_sqs, const size_t *counts, int nb,
                                      KungFu_Datatype dt, int np, const kf_adam_hyper *hyper,
                                      const kf_step_gate *gate, const kf_step_state *state,
                                      void *stream);

/* ---- Adam, stochastic rounding: bf16 parameters and state, fp32 registers --
 *
 * The third choice for a bf16 model beside kf_adam_update_batch (bf16 state,
 * every operation rounded to nearest even: an update below half an ulp of p is
 * rounded away, and rnd(b2*v) == v for every normal v at beta2 = 0.999, so
 * exp_avg_sq never decays) and kf_adam_master_update_batch (28 bytes per
 * element, 12 bytes of state): kungfu_amd/csrc/kf_adam_sr.hip, DESIGN.md §18.
 * 14 bytes per element and 4 bytes of state, as the first; both stalls go
 * away in expectation.
 *
 * Arithmetic. kf_adam_update_batch's f32 arithmetic, operation for operation,
 * on the widened bf16 p, g, m and v: exactly what kf_adam_master_update_batch
 * runs on its master. The widening is exact, the /np is the fp32 one, and no
 * intermediate value is rounded to 16 bits; p', m', v' are the f32 results.
 *
 * Stores.  p = sr(p', r_p);  m = f32_to_bf16(m') (round-to-nearest-even: m
 * decays by 10 % a step and cannot stall);  v = sr(v', r_v).
 *
 * sr(x, r), for a finite x and 16 random bits r, is
 *   (bits(x) + r) >> 16                  as unsigned 32-bit arithmetic,
 * that is, x goes to the next bf16 away from zero with probability
 * low16(bits(x)) / 2^16 and is truncated otherwise: E[sr(x)] = x. A carry into
 * the exponent is kept, so a finite f32 above bf16's largest finite value may
 * become inf. A value that is exactly a bf16 is returned unchanged for every
 * r. inf and NaN narrow as the round-to-nearest-even narrowing does (inf
 * stays; a NaN keeps its sign and upper payload and is made quiet).
 *
 * Random bits: a pure function of (key, stream word, element index). They do
 * not depend on the launch geometry, on how the elements are split into
 * segments, on the rank or on the world. For element i of segment b, with
 * e = bases[b] + i:
 *   (a, b) = philox2x32_10(c0 = (uint32_t)(e >> 1), c1 = streams[b], key)
 *   w = (e & 1) ? b : a;   r_p = w >> 16;   r_v = w & 0xffff
 * Philox2x32-10 (Salmon, Moraes, Dror, Shaw 2011): ten rounds of
 *   (hi, lo) = 0xD256D193 * c0 (64-bit product);  c0 = hi ^ key ^ c1;  c1 = lo
 * with key = key + 0x9E3779B9 between rounds. Known answers (c0, c1, key ->
 * a, b): (0, 0, 0 -> ff1dae59, 6cd10df2), (ffffffff, ffffffff, ffffffff ->
 * 2c3f628b, ab4fd7ad), (243f6a88, 85a308d3, 13198a2e -> dd7ce038, f62a4c12).
 * One evaluation serves an element pair.
 *
 * kf_adam_sr_update_batch takes what kf_adam_update_batch takes, plus per
 * segment bases[b] (the element index of its first element) and streams[b],
 * and one key for the call. kf_adam_sr_update_batch_gated follows
 * kf_adam_update_batch_gated's rules: one hyper, a skipped step returns before
 * any load and leaves every byte as it was, grad_mul, s2 and nss come from the
 * device. Checks, all before any HIP call: everything kf_adam_update_batch
 * checks (bases and streams are tables like the others); dt must be
 * KungFu_BFLOAT16 (KF_ERR_DTYPE otherwise); in a non-empty segment bases[b]
 * must be a multiple of 8 and bases[b] + counts[b] at most 2^33 (KF_ERR_ARG).
 * One launch per 32 segments.
 *
 * kf_adam_sr_narrow is sr() alone: out[i] = sr(x[i], r[i]) for n fp32 bit
 * patterns x, n 16-bit words r and n bf16 results, all on the device. It runs
 * the update kernels' own narrowing and exists so that the narrowing can be
 * swept over its whole domain. */
int kf_adam_sr_update_batch(void *const *params, const void *const *grads, void *const *exp_avgs,
                            void *const *exp_avg_sqs, const size_t *counts, const uint64_t *bases,
                            const uint32_t *streams, int nb, KungFu_Datatype dt, int np,
                            const kf_adam_hyper *hyper, uint32_t key, void *stream);
int kf_adam_sr_update_batch_gated(void *const *params, const void *const *grads,
                                  void *const *exp_avgs, void *const *exp_avg_sqs,
                                  const size_t *counts, const uint64_t *bases,
                                  const uint32_t *streams, int nb, KungFu_Datatype dt, int np,
                                  const kf_adam_hyper *hyper, uint32_t key,
                                  const kf_step_gate *gate, const kf_step_state *state,
                                  void *stream);
int kf_adam_sr_narrow(const void *x, const void *r, void *out, size_t n, void *stream);

/* ---- Adam, 8-bit block-wise state ------------------------------------------
 *
 * exp_avg and exp_avg_sq held as one uint8 code per element and one f32 scale
 * per block of 64 consecutive elements (Dettmers et al., "8-bit Optimizers via
 * Block-wise Quantization"): 2.125 bytes of state per element where
 * kf_adam_update_batch keeps 8, and 16.25 bytes of kernel traffic where it
 * moves 28 (kungfu_amd/csrc/kf_adam8.hip).
 *
 * The format, for one block x[0..64) of f32 values and one of two tables T of
 * 256 f32 values (kf_adam8_codebook: which = 0 the signed table of exp_avg,
 * which = 1 the unsigned table of exp_avg_sq), sorted ascending, with
 * mid[k] = (float)(((double)T[k] + (double)T[k+1]) / 2), k = 0..254:
 *   mag = max |x_j|;  a = +mag if some x_j == +mag, else -mag;
 *   a = NaN (0x7FC00000) if any x_j is NaN           the block's scale
 *   y_j = a == 0 ? 0 : x_j / a                       correctly rounded
 *   code_j = the number of k with mid[k] < y_j       (a NaN y: 0)
 *   x_j' = T[code_j] * a                             dequantized, one multiply
 * The element of largest magnitude has code 255 (T[255] = 1) and comes back
 * exactly. Infinities follow from IEEE arithmetic on these formulas. A zeroed
 * state is scale 0 with code 127 (signed) or 0 (unsigned): not all zero bytes.
 *
 * The tables, built in double and rounded once to f32. Decade i = 0..6 has n_i
 * equal intervals on [0.1, 1], b_k = 0.1 + 0.9*k/n_i, and the values
 * 10^(i-6) * (b_k + b_{k+1}) / 2. Signed: n_i = 2^i, both signs, 0 and 1 (127
 * + 127 + 2 values; T[0] = -0.99296874, T[127] = 0, T[254] = 0.99296874).
 * Unsigned: n_i = 2^(i+1), 0 and 1 (254 + 2 values; T[1] = 3.25e-07, T[254] =
 * 0.9964844).
 *
 * The update of a block: dequantize m and v, run kf_adam_update_batch's f32
 * arithmetic on them operation for operation (kf_adam_master_update_batch's
 * for 16-bit parameters: the f32 update on the master, params16 = the master
 * narrowed), the parameter from the unquantized new m and v, then quantize the
 * new m and v. Gradients are only read. Nothing is written beyond counts[b]
 * parameters, counts[b] code bytes and counts[b] / 64 scales per state.
 *
 * kf_adam8_update_batch: f32 parameters and gradients. m_codes[b] / v_codes[b]
 * hold counts[b] bytes, m_scales[b] / v_scales[b] counts[b] / 64 floats.
 * kf_adam8_master_update_batch: bf16 or f16 params16 (written, never read) and
 * grads16, f32 masters. The _gated twins follow kf_adam_update_batch_gated's
 * rules: one hyper, grad_mul, s2 and nss from the device, and a skipped step
 * returns before any load and leaves every byte of the parameters, masters,
 * codes and scales as it was. Checks, all before any HIP call: null tables or
 * pointers of a non-empty segment, np < 0, bias corrections <= 0, a gate or a
 * state missing (KF_ERR_ARG); dt other than KungFu_FLOAT, or for the master
 * entries other than KungFu_BFLOAT16 / KungFu_FLOAT16 (KF_ERR_DTYPE);
 * parameter, gradient, master and codes pointers 16-byte aligned, scales
 * pointers 4-byte aligned, counts[b] a multiple of 64 (KF_ERR_ARG): there is
 * no scalar tail. One launch per 24 segments.
 *
 * kf_adam8_quantize / kf_adam8_dequantize are the format alone on the device,
 * n a multiple of 64 f32 values, for the checkpoint path and for sweeping the
 * quantizer's domain: src / dst and codes 16-byte aligned, scales 4-byte
 * aligned, which 0 or 1 (KF_ERR_ARG otherwise). Requantizing a dequantized
 * block gives the same codes and scale, except where |scale| is so small that
 * T[c] * a is subnormal. kf_adam8_codebook writes table `which` to the host
 * array out[256] and needs no device. */
int kf_adam8_codebook(int which, float *out);
int kf_adam8_update_batch(void *const *params, const void *const *grads, void *const *m_codes,
                          void *const *v_codes, void *const *m_scales, void *const *v_scales,
                          const size_t *counts, int nb, KungFu_Datatype dt, int np,
                          const kf_adam_hyper *hyper, void *stream);
int kf_adam8_update_batch_gated(void *const *params, const void *const *grads,
                                void *const *m_codes, void *const *v_codes,
                                void *const *m_scales, void *const *v_scales,
                                const size_t *counts, int nb, KungFu_Datatype dt, int np,
                                const kf_adam_hyper *hyper, const kf_step_gate *gate,
                                const kf_step_state *state, void *stream);
int kf_adam8_master_update_batch(void *const *params16, const void *const *grads16,
                                 void *const *masters, void *const *m_codes, void *const *v_codes,
                                 void *const *m_scales, void *const *v_scales,
                                 const size_t *counts, int nb, KungFu_Datatype dt, int np,
                                 const kf_adam_hyper *hyper, void *stream);
int kf_adam8_master_update_batch_gated(void *const *params16, const void *const *grads16,
                                       void *const *masters, void *const *m_codes,
                                       void *const *v_codes, void *const *m_scales,
                                       void *const *v_scales, const size_t *counts, int nb,
                                       KungFu_Datatype dt, int np, const kf_adam_hyper *hyper,
                                       const kf_step_gate *gate, const kf_step_state *state,
                                       void *stream);
int kf_adam8_quantize(const void *src, void *codes, void *scales, size_t n, int which,
                      void *stream);
int kf_adam8_dequantize(const void *codes, const void *scales, void *dst, size_t n, int which,
                        void *stream);

/* ---- LAMB: layer-wise trust ratios on the sharded step --------------------
 *
 * LAMB (kungfu_amd/csrc/kf_lamb.hip) where the averaged
 * gradient, exp_avg and exp_avg_sq only exist as one rank's shard and a tensor
 * straddles shard boundaries at element offsets. A step is two element-wise
 * passes with the norms between them. Every parenthesis is one IEEE operation
 * in the compute type C, no FMA contraction; the sqrt and the divisions are
 * correctly rounded; scalars are computed in double and cast once to C, as
 * kf_adam_update_batch does. C is f32 for f32 parameters and f64 for f64; for
 * bf16 / f16 parameters C is f32 on the fp32 master copy.
 *
 * Pass 1, moments, per element of this rank's shard:
 *   g = np > 0 ? g / np : g                     (kf_bucket_div's rounding, as Adam)
 *   m = (b1*m) + (c1*g)                         c1 = 1 - beta1
 *   v = (b2*v) + (c2*(g*g))                     c2 = 1 - beta2
 *   d = (sqrt(v) / s2) + eps                    s2 = sqrt(bias_correction2)
 *   u = rb1 * (m / d)                           rb1 = (C)(1 / bias_correction1)
 *   weight_decay != 0:  u = u + (wd*p)
 * p is read and not written; m, v and u are written; u is a scratch shard of
 * type C beside the state shards, never the gradient's own storage. 7 accesses
 * per element: 28 bytes for f32, 26 on the master path (g is 2 bytes there).
 *
 * Norms: one kf_segnorm plan (below) of 2T segments on every rank, T the
 * number of tensors: segment t is the piece of tensor t's parameters (of its
 * master copy, on the master path) that lies in this rank's shard, with count
 * 0 where the rank holds none of it; segment T + t is the same piece of u.
 * out[0 .. 2T) is this rank's send vector of kf_exchange_all_gather_doubles,
 * which gives sq[r][k].
 *
 * Trust, one lane per tensor, fp64:
 *   P = 0; for r in rank order: P = P + sq[r][t]      U likewise from sq[r][T + t]
 *   wn = sqrt(P); un = sqrt(U)
 *   ratio = (adapt_t && wn > 0 && un > 0) ? wn / un : 1
 *   trust_clip > 0:  ratio = ratio < trust_clip ? ratio : trust_clip
 *   nlr[t] = -(lr_t * ratio); ratio[t] = ratio
 * lr_t and adapt_t are those of tensor t's group, groups[group_of[t]].
 *
 * Pass 2, apply, per element of a piece:  p = p + ((C)nlr[t] * u); on the
 * master path the same on the master, and params16 = narrow(master),
 * round-to-nearest-even. Elements outside every piece (bucket padding) are not
 * touched. 3 accesses per element.
 *
 * Non-finite gradients are NOT skipped: an inf or a NaN in a gradient reaches
 * m, v, u, the tensor's norms and through them its parameters, as it does in
 * torch.optim.Adam. There is no gate on this path; the entries under a gate
 * are "LAMB under a gate" below. */

/* The moments pass over nb segments of one dtype, one launch per 24 of them
 * (f32, f64) or per 32 (master path). kf_adam_update_batch's conventions:
 * every pointer 16-byte aligned, segment b has counts[b] elements and its own
 * hyper[b], whose lr and decoupled are ignored; bias corrections must be > 0.
 * kf_lamb_moments_batch takes f32 and f64 (anything else, bf16 and f16 among
 * them: KF_ERR_DTYPE); params, grads, exp_avgs, exp_avg_sqs and updates all
 * have that type. kf_lamb_master_moments_batch takes dt = bf16 or f16, the
 * type of grads16 alone: masters, exp_avgs, exp_avg_sqs and updates are fp32.
 * params / masters and the gradients are only read. */
int kf_lamb_moments_batch(const void *const *params, const void *const *grads,
                          void *const *exp_avgs, void *const *exp_avg_sqs, void *const *updates,
                          const size_t *counts, int nb, KungFu_Datatype dt, int np,
                          const kf_adam_hyper *hyper, void *stream);
int kf_lamb_master_moments_batch(const void *const *grads16, const void *const *masters,
                                 void *const *exp_avgs, void *const *exp_avg_sqs,
                                 void *const *updates, const size_t *counts, int nb,
                                 KungFu_Datatype dt, int np, const kf_adam_hyper *hyper,
                                 void *stream);

/* The trust ratios of ntensor tensors. sq is a device array of world * 2 *
 * ntensor doubles, sq[r * 2 * ntensor + k]; group_of (device, ntensor ints,
 * uploaded once by the caller) maps a tensor to its group; groups (host,
 * ngroup entries, read before the call returns) come with every call because
 * schedulers change lr. nlr and ratio are device arrays of ntensor doubles.
 * A tensor whose group index is outside [0, ngroup) is not written. Any
 * ntensor >= 1, world >= 1 and ngroup >= 1: one launch per 16 groups, on the
 * same stream. trust_clip <= 0 means no clipping. No atomics, no host sync,
 * no allocation. */
typedef struct { double lr; int adapt; } kf_lamb_group;
int kf_lamb_trust_update(const double *sq, int world, int ntensor, const int *group_of,
                         const kf_lamb_group *groups, int ngroup, double trust_clip, double *nlr,
                         double *ratio, void *stream);

/* The apply pass as a plan (kf_segnorm's shape): kf_lamb_apply_create uploads
 * the piece table to HBM once; kf_lamb_apply_run is one launch whatever the
 * number of pieces, and only queues it (no allocation, no host sync). Piece i
 * is counts[i] elements at params[i] and updates[i] of dt (f32 or f64,
 * params16 == NULL), or, with dt = bf16 / f16, fp32 elements at params[i] (the
 * master) and updates[i] and 16-bit ones at params16[i]; tensors[i] in
 * [0, ntensor) indexes nlr. Pointers are aligned to the element only, but a
 * piece's arrays must share their element offset from a 16-byte boundary
 * (KF_ERR_ARG otherwise; pieces cut from shards that start 16-byte aligned
 * do). A count may be 0 and npiece may be 0. Returns NULL on failure with
 * kf_last_error() set. nlr is kf_lamb_trust_update's, ntensor doubles. */
typedef struct kf_lamb_apply kf_lamb_apply_t; /* opaque plan */
kf_lamb_apply_t *kf_lamb_apply_create(void *const *params, const void *const *updates,
                                      void *const *params16 /* NULL: f32, f64 */,
                                      const size_t *counts, const int *tensors, int npiece,
                                      int ntensor, KungFu_Datatype dt);
int kf_lamb_apply_run(kf_lamb_apply_t *p, const double *nlr, void *stream);
void kf_lamb_apply_destroy(kf_lamb_apply_t *p);

/* ---- LAMB under a gate: clipping, loss scale and skipped steps -------------
 *
 * The LAMB step above under the gated step's verdict (kf_step_gate_update,
 * DESIGN.md §19): kernels of their own beside the parents' in kf_lamb.hip,
 * through the parents' bodies. A step is
 *   A  every group: the exchange's reduce of the gradients to this rank's shards
 *   B  per dtype: kf_segnorm over this rank's gradient shards -> one fp64 sum
 *   C  kf_exchange_all_gather_doubles of those sums
 *   D  kf_step_gate_update, unchanged, called with every group's lr = 1.0
 *   E  every group: the gated moments pass
 *   F  per (dtype, device): the norm plan over the 2T (p, u) pieces and the
 *      all-gather of its sums, as without a gate
 *   G  the gated trust update; the gated apply run
 *   H  every group: the all-gather of the parameters
 * all queued on one stream; nothing is allocated per step and the host never
 * waits for the verdict.
 *
 * D, the lr = 1 rule. kf_step_state.nss_f64 is -(lr / (1 - beta1_pow)); with
 * lr = 1 it is -(1 / bias_correction1). The gated moments kernel takes
 * rb1 = -nss (nss_f64 for f64, nss otherwise) and s2 from the state. Negation
 * is exact and the cast to fp32 commutes with it, so rb1 equals the ungated
 * (C)(1 / bias_correction1) bit for bit whenever bias_correction1 ==
 * 1 - beta1_pow. The real lr goes to the trust update only, as without a gate.
 *
 * E. Every block reads gate->skip; on a skipped step the kernel returns before
 * touching exp_avgs, exp_avg_sqs, updates, params or masters. Otherwise it is
 * pass 1 above with exactly one operation inserted directly after the /np:
 *   g = (g * grad_mul)
 * rounded to C (f32 on the master path), and with s2 and rb1 from *state. ONE
 * hyper serves the whole call; its lr, decoupled and bias corrections are
 * ignored (kf_adam_update_batch_gated's rule).
 *
 * F runs unconditionally: it only reads, and on a skipped step it reads the
 * previous u.
 *
 * G. kf_lamb_trust_update_gated returns on skip and leaves nlr[] and ratio[] as
 * they were: they describe the last applied step. kf_lamb_apply_run_gated
 * returns on skip before any load of the table, params, updates or params16.
 * Otherwise both are their parents' arithmetic, operation for operation.
 *
 * A skipped step leaves every byte of params, params16, masters, exp_avgs,
 * exp_avg_sqs, updates, nlr, ratio and every group's step state as it was; the
 * loss scale and the counters follow kf_step_gate_update's rule.
 *
 * Checks, all before any HIP call: the parents', plus gate and state not NULL
 * (KF_ERR_ARG). gate and state are device pointers written by an earlier
 * kf_step_gate_update on the same stream; state is the segments' group's. */
int kf_lamb_moments_batch_gated(const void *const *params, const void *const *grads,
                                void *const *exp_avgs, void *const *exp_avg_sqs,
                                void *const *updates, const size_t *counts, int nb,
                                KungFu_Datatype dt, int np, const kf_adam_hyper *hyper,
                                const kf_step_gate *gate, const kf_step_state *state, void *stream);
int kf_lamb_master_moments_batch_gated(const void *const *grads16, const void *const *masters,
                                       void *const *exp_avgs, void *const *exp_avg_sqs,
                                       void *const *updates, const size_t *counts, int nb,
                                       KungFu_Datatype dt, int np, const kf_adam_hyper *hyper,
                                       const kf_step_gate *gate, const kf_step_state *state,
                                       void *stream);
int kf_lamb_trust_update_gated(const double *sq, int world, int ntensor, const int *group_of,
                               const kf_lamb_group *groups, int ngroup, double trust_clip,
                               double *nlr, double *ratio, const kf_step_gate *gate, void *stream);
int kf_lamb_apply_run_gated(kf_lamb_apply_t *p, const double *nlr, const kf_step_gate *gate,
                            void *stream);

/* ---- gradient monitors: segmented squared norms ------------------------- */

/* What MonitorGradientNoiseScaleOptimizer and MonitorGradientVarianceOptimizer
 * (grad_noise_scale.py, grad_variance.py) need beyond the sync reduce: many
 * tensors, each reduced to one fp64 scalar, in one read-only pass.
 *
 * A plan holds nseg segments: a[s] (and b[s], or b == NULL for a plan that
 * only runs KF_NORM_SQ), counts[s] elements of `dt` (f32, f16, bf16 or f64;
 * anything else: KF_ERR_DTYPE). Pointers are device pointers aligned to the
 * element size only; a count may be 0; nseg >= 1 with no upper limit.
 * kf_segnorm_create uploads the segment table to HBM and allocates the
 * per-block partials workspace on the current device (once per optimizer:
 * bucket views never move). It returns NULL on failure, with kf_last_error()
 * starting with the status name ("KF_ERR_ARG: ...").
 *
 * kf_segnorm_run only queues launches on `stream`: no allocation, no host
 * sync, safe to capture into a hipGraph. It writes nseg + 1 doubles to the
 * device array `out`:
 *   KF_NORM_SQ   out[s] = sum_i a_s[i]^2
 *   KF_NORM_VAR  out[s] = sum_i d_i^2, d_i = fl_T(a_s[i] - fl_T(b_s[i] * b_s[i]))
 *                (square_grad - tf.square(grad), grad_variance.py:51-54, in the
 *                tensors' own dtype T: every operation rounded to T, no FMA
 *                contraction; f16 / bf16 compute in fp32 and round to T after
 *                the multiply and after the subtract). Needs b: KF_ERR_ARG.
 *   out[nseg]    = out[0] + out[1] + ... left to right in fp64, or with
 *                KF_NORM_TOTAL_SQRT or-ed into the mode the same sum of
 *                sqrt(out[s]) (sum_t ||var_t||, grad_variance.py:55-58).
 * Accumulation is fp64 from the first add: |out[s] - exact_s| <=
 * (n_s + 2) * 2^-53 * exact_s; fp32 inputs near FLT_MAX do not overflow and
 * fp32 subnormals are not flushed. A count of 0 gives 0.0. The same plan and
 * the same input bytes give the same output bits on every run (no atomics;
 * partials are combined in a fixed order after a launch boundary).
 * A plan's workspace serves one run at a time in stream order: runs of one
 * plan on two streams at once are the caller's to order. */
typedef struct kf_segnorm kf_segnorm_t; /* opaque plan */
enum { KF_NORM_SQ = 0, KF_NORM_VAR = 1 }; /* mode */
#define KF_NORM_TOTAL_SQRT 0x100 /* or-ed into mode */

kf_segnorm_t *kf_segnorm_create(const void *const *a, const void *const *b /* NULL: SQ only */,
                                const size_t *counts, int nseg, KungFu_Datatype dt);
int kf_segnorm_run(kf_segnorm_t *p, int mode, double *out /* device, nseg + 1 */, void *stream);
void kf_segnorm_destroy(kf_segnorm_t *p);

/* The gradient noise scale's running estimate, on the device so that a
 * monitored step needs no host sync (monitor.py:10-17, ema.hpp:19-27,
 * collective.cpp:298-300; fp32, no contraction, one lane):
 *   Gs = (float)*sq_small, Gb = (float)*sq_big
 *   G = (1 / (bb - bs)) * (bb * Gb - bs * Gs)
 *   S = (1 / (1 / bs - 1 / bb)) * (Gs - Gb)
 *   each EMA: x on its first update, else alpha * v + (1 - alpha) * x
 *   noise_scale = s_ema / g_ema
 * state is 4 device floats {g_ema, s_ema, noise_scale, has_value}; all zero
 * means "no value yet". bb == bs (one peer) follows IEEE (inf or NaN), as the
 * reference. alpha <= 0: KF_ERR_ARG (collective.cpp:283). */
int kf_noise_scale_update(const double *sq_small, const double *sq_big, float batch_small,
                          float batch_big, float alpha, float *state, void *stream);

/* ---- runtime / diagnostics ---------------------------------------------- */

/* HIP device count visible to the library (0 on a GPU-less host). */
int kf_device_count(void);

/* Library/ABI version string. */
const char *kf_version(void);

/* Last HIP error string recorded by the library on this thread. */
const char *kf_last_error(void);

/* Release the library's process-wide HIP resources (the streams and HBM
 * scratch std_transform_2 / kf_transform2_host lend to their calls) while the
 * HIP runtime is still up. No destructor in the library calls HIP at process
 * exit, so a host that never calls this leaves those to the OS. Call it once
 * no host-API call is running (KF_ERR_ARG otherwise: the busy ones are kept);
 * the library stays usable afterwards. The Python binding calls it at
 * interpreter exit. */
int kf_shutdown(void);

/* kf_bucket_reduce / kf_bucket_reduce_avg for inputs that sit behind
 * different links (kungfu_amd/p2p.py: shard `rank` of every peer's bucket,
 * mapped over xGMI): every thread has the loads of up to 8 inputs in flight
 * before the first add, so all links carry traffic at once; the fold order is
 * still inputs[0], inputs[1], ... (bit-identical result). np > 0: SUM then
 * / np (float dtypes); np == 0: the plain op. Same contract as B2. */
int kf_bucket_reduce_peers(const void *const *inputs, int k, void *out, size_t n,
                           KungFu_Datatype dt, KungFu_Op op, int np, void *stream);

/* Page-lock / release a host range so std_transform_2 and
 * kf_transform2_host can DMA it directly (e.g. a receive-buffer pool the
 * transport reuses, srcs/go/rchannel/connection/byte_slice_pool.go:28-60).
 * The library remembers the range (a chunk inside it needs no pointer
 * queries); release it with kf_host_unregister(p), p the registered base. */
int kf_host_register(void *p, size_t bytes);
int kf_host_unregister(void *p);

/* Tuning hook (tools/tune_reduce.py only): launch geometry of the fp32 SUM
 * 2-input path — unroll in {1,2,4,8} vectors per thread, grid cap in blocks,
 * non-temporal loads, plain stores. Not thread-safe; call before launching. */
int kf_set_geometry(int unroll, int grid_cap, int loadnt, int stplain);
/* Tuning hook (A/B tools only): occupancy cap of the HBM streaming kernels
 * (kf_bucket_reduce*, kf_bucket_div, kf_sma_blend; not the batched launch), as
 * dynamic LDS bytes per 256-thread block (0 = none, at most 64 KiB) for the
 * k <= 2 kernels (two-input sum, /np, SMA) and for the k >= 3 folds.
 * Defaults: 0 and 32 KiB (five blocks per CU); the fold's cap applies to
 * launches of at least 8192 blocks (128 MiB per fp32 input). Not thread-safe. */
int kf_set_occupancy(int lds_small, int lds_fold);

/* Host-pointer reduce with a status code instead of exit(): the path
 * std_transform_2 takes. Synchronous, a stream and device scratch lent to the
 * call from a process-wide pool (kf_shutdown frees them).
 * If x, y and out are all device-accessible (page-locked by hipHostMalloc or
 * kf_host_register, or HBM of the current device) the kernel reads and writes
 * them in place (zero copy, over PCIe for host memory); otherwise pageable
 * copies through the runtime's staging to HBM scratch and back. Used by the
 * copy-inclusive measurement (bench.py host_staged). */
int kf_transform2_host(const void *x, const void *y, void *out, size_t n,
                       KungFu_Datatype dt, KungFu_Op op);

/* ---- host ingestion: rchannel wire format + device recvOnto ----------- */

/* rchannel constants (srcs/go/rchannel/connection/message.go:10-17, 71-78) */
#define KF_RCH_CONN_COLLECTIVE 2
#define KF_RCH_NO_FLAG 0u
#define KF_RCH_WAIT_RECV_BUF 1u

/* Connection handshake: client sends {u16 type, u16 src_port, u32 src_ipv4},
 * server answers {u32 token}; a token mismatch on a collective connection is
 * an error (srcs/go/rchannel/connection/connection.go:28-101). */
int kf_rch_client_handshake(int fd, uint16_t conn_type, uint16_t src_port,
                            uint32_t src_ipv4, uint32_t expect_token);
int kf_rch_server_handshake(int fd, uint32_t token, uint16_t *conn_type,
                            uint16_t *src_port, uint32_t *src_ipv4);

/* One named message: {u32 name_len, name, u32 flags} {u32 len, payload}
 * (message.go:90-198; tcpConnection.Send, connection.go:149-165). */
int kf_rch_send(int fd, const char *name, uint32_t flags, const void *data,
                uint32_t len);
/* Reads a message header; name is NUL-terminated into name[cap]. */
int kf_rch_recv_header(int fd, char *name, uint32_t cap, uint32_t *name_len,
                       uint32_t *flags);
/* Reads a message body into dst; its length must equal expect_len
 * (Message.ReadInto, message.go:184-198). */
int kf_rch_recv_body(int fd, void *dst, uint32_t expect_len);

/* Page-locked landing slots + device slots for peer chunks. */
#pragma GCC visibility pop
typedef struct kf_ingest kf_ingest_t; /* opaque; its C++ body stays hidden */
#pragma GCC visibility push(default)
kf_ingest_t *kf_ingest_create(size_t slot_bytes, int nslots);
void kf_ingest_destroy(kf_ingest_t *g);

/* recvOnto on the device (session.go:255-264): read the body of the message
 * whose header was just read (len bytes) from fd into the next page-locked
 * slot, then on `stream`: copy it to HBM and fold dev_acc = own o peer, with
 * own = dev_own (SendBuf before the first receive) or dev_acc if NULL.
 * Returns after the socket read; the device work stays queued on `stream`. */
int kf_ingest_recv_onto(kf_ingest_t *g, int fd, uint32_t len, void *dev_acc,
                        const void *dev_own, size_t count, KungFu_Datatype dt,
                        KungFu_Op op, void *stream);
/* recvInto on the device (session.go:266-270): read the body into the next
 * page-locked slot and queue its copy into dev_dst on `stream`. */
int kf_ingest_recv_into(kf_ingest_t *g, int fd, uint32_t len, void *dev_dst,
                        void *stream);
/* The same two steps with the body read in pieces of piece_bytes (a multiple
 * of the element size): each piece's fold (or copy) is queued on `stream` as
 * soon as that piece has been read, so the device work of a chunk overlaps
 * the rest of its socket read. piece_events (hipEvent_t handles, may be NULL;
 * at least ceil(len / piece_bytes) of them) gets event k recorded after piece
 * k's fold. Element-wise, so the bits equal the whole-chunk call's. */
int kf_ingest_recv_onto_pieces(kf_ingest_t *g, int fd, uint32_t len, void *dev_acc,
                               const void *dev_own, size_t count, KungFu_Datatype dt,
                               KungFu_Op op, void *stream, uint32_t piece_bytes,
                               void *const *piece_events, int n_events);
int kf_ingest_recv_into_pieces(kf_ingest_t *g, int fd, uint32_t len, void *dev_dst,
                               void *stream, uint32_t piece_bytes);
/* sendOnto/sendInto from the device: copy bytes of dev_src (after the work
 * queued on `stream`) to a page-locked slot and send it as one message. */
int kf_ingest_send_from_device(kf_ingest_t *g, int fd, const char *name,
                               uint32_t flags, const void *dev_src, size_t bytes,
                               void *stream);
/* The same two steps for a chunk already in host memory (a message read
 * ahead of its all-reduce and kept, as the reference's per-name mailbox
 * does, handler/collective.go:27-41). */
int kf_ingest_fold_host(kf_ingest_t *g, const void *host, uint32_t len,
                        void *dev_acc, const void *dev_own, size_t count,
                        KungFu_Datatype dt, KungFu_Op op, void *stream);
int kf_ingest_copy_host(kf_ingest_t *g, const void *host, uint32_t len,
                        void *dev_dst, void *stream);
/* Wait for every queued slot copy. */
int kf_ingest_sync(kf_ingest_t *g);
const char *kf_ingest_last_error(void);

/* ---- session engine (collective boundary) ---------------- */

/* Host-mode fold callback: out = x op y over n elements; 0 = ok. */
typedef int (*kf_host_reduce_fn)(const void *x, const void *y, void *out,
                                 int64_t n, int dt, int op);

#pragma GCC visibility pop
typedef struct kf_session kf_session_t; /* opaque; its C++ body stays hidden */
#pragma GCC visibility push(default)

/* Peer `rank` of `size` on this host: listens on
 * <sock_dir>/kungfu-amd-127.0.0.1-<10000+rank>.sock and connects to every other peer
 * (rchannel handshake with `token`). The strategy and chunk hash come from
 * KUNGFU_ALLREDUCE_STRATEGY / KUNGFU_CONFIG_STRATEGY_HASH_METHOD as in the
 * reference (default BINARY_TREE_STAR, NAME). device_mode = 1: buffers passed
 * to kf_session_all_reduce are HBM pointers; 0: host pointers. NULL on
 * failure (kf_session_last_error). */
kf_session_t *kf_session_create(int rank, int size, const char *sock_dir,
                                uint32_t token, int device_mode);
/* Peer `self_spec` of the cluster `peer_list`, in the formats kungfu-run
 * exports as KUNGFU_SELF_SPEC / KUNGFU_INIT_PEERS ("ipv4:port" and a
 * comma-separated list of them, plan/id.go:34-50, plan/peerlist.go:180-192);
 * the rank is self's index in the list. Peers with the same IPv4 connect over
 * <sock_dir>/kungfu-amd-<ipv4>-<port>.sock, the others over TCP to ipv4:port
 * (rchannel/connection/connection.go:58-64); every peer listens on its own
 * address. Multi-host strategies (TREE, BINARY_TREE_STAR, MULTI_*, AUTO ->
 * BINARY_TREE_STAR) follow the hosts (plan/topology.go:5-136). */
kf_session_t *kf_session_create_peers(const char *peer_list, const char *self_spec,
                                      const char *sock_dir, uint32_t token,
                                      int device_mode);
/* Override the strategy (KungFu_Strategy) and chunk hash (1 = NAME,
 * 0 = SIMPLE); every peer must use the same. */
int kf_session_set_strategy(kf_session_t *s, int strategy, int hash_by_name);
/* Host mode only: fold with `fn` instead of std_transform_2. */
int kf_session_set_host_reduce(kf_session_t *s, kf_host_reduce_fn fn);
/* Synchronous all-reduce of one bucket: the counterpart of
 * GoKungfuAllReduce(sendBuf, recvBuf, count, dtype, op, name, done = nil)
 * (srcs/go/libkungfu-comm/collective.go:34-45). send == recv is in place.
 * Every peer must call it with the same name, count, dtype and op. */
int kf_session_all_reduce(kf_session_t *s, const void *send, void *recv,
                          size_t count, KungFu_Datatype dt, KungFu_Op op,
                          const char *name, void *stream);
/* GoKungfuSubsetAllReduce (srcs/go/libkungfu-comm/collective.go:47-60) ->
 * Session.SubsetAllReduce (srcs/go/kungfu/session/allreduce.go:14-24): every
 * tree of the forest all-reduces within itself. forest[i] = i's father, a
 * root is its own (graph.go:46-62); size entries. Chunked like the
 * all-reduce, one strategy (reduce = reversed tree with self loops, bcast =
 * the tree). A lone node forwards its send. KF_ERR_ARG for an index out of
 * range or a cycle. */
int kf_session_subset_all_reduce(kf_session_t *s, const void *send, void *recv, size_t count,
                                 KungFu_Datatype dt, KungFu_Op op, const int32_t *forest,
                                 const char *name, void *stream);
/* GoKungfuReduce (srcs/go/libkungfu-comm/collective.go:109-120) ->
 * Session.Reduce (srcs/go/kungfu/session/session.go:159-162): the reduce graph
 * of the session's first strategy only. The graph's root ends with the
 * reduction in recv; an inner node with its partial fold; a leaf's recv is
 * left as it was (runGraphs forwards only in a graph without self loops),
 * unless the peer is alone. Same fold order rules as the all-reduce. */
int kf_session_reduce(kf_session_t *s, const void *send, void *recv, size_t count,
                      KungFu_Datatype dt, KungFu_Op op, const char *name, void *stream);
/* GoKungfuBroadcast (collective.go:122-132) -> Session.Broadcast
 * (session.go:164-167): the first strategy's bcast graph; every peer's recv
 * becomes the root's send (the root forwards its own). */
int kf_session_broadcast(kf_session_t *s, const void *send, void *recv, size_t count,
                         KungFu_Datatype dt, const char *name, void *stream);
/* GoKungfuAllReduce with done != nil (srcs/go/libkungfu-comm/collective.go:
 * 34-45, main.go:184-191): start the all-reduce on the session's worker
 * thread and return KF_OK at once; done(status, arg) runs on that thread when
 * it has finished (the reference drops the error, main.go:188; here it is
 * passed on). Every started all-reduce is in flight at once in the worker's
 * poll loop and peers' chunks pair by name, as with the reference's goroutine
 * per call (rchannel/handler/collective.go:48-64), so peers may start their
 * names in different orders; done callbacks come in completion order. A name
 * started while its previous call is in flight waits for it (the next step's
 * call of the same name). Buffers stay valid and untouched until done; the
 * name is copied. A synchronous
 * kf_session_all_reduce first waits for everything queued before it; from
 * inside a done callback it (and kf_session_wait_all) returns KF_ERR_ARG
 * instead of waiting for itself. */
typedef void (*kf_done_fn)(int status, void *arg);
int kf_session_all_reduce_async(kf_session_t *s, const void *send, void *recv,
                                size_t count, KungFu_Datatype dt, KungFu_Op op,
                                const char *name, void *stream, kf_done_fn done,
                                void *arg);
/* Block until every queued all-reduce has finished; the first failure since
 * the previous wait (its message in kf_session_last_error), else KF_OK. */
/* Barrier (GoKungfuBarrier, libkungfu-comm/collective.go:17-20; session.go:
 * 104-115): an all-reduce of size() zero bytes every peer joins. Blocking;
 * device-mode sessions use a workspace of their own in HBM. */
int kf_session_barrier(kf_session_t *s);
int kf_session_wait_all(kf_session_t *s);
/* Peer::Rank / Size / LocalRank / LocalSize / HostCount (include/kungfu/
 * peer.hpp): peers with the same IPv4 share a host; local ranks follow the
 * peer list's order. Any pointer may be NULL. */
int kf_session_info(kf_session_t *s, int *rank, int *size, int *local_rank, int *local_size,
                    int *host_count);
void kf_session_destroy(kf_session_t *s);
const char *kf_session_last_error(void);

/* ---- peer-to-peer over xGMI (kungfu_amd/p2p.py) ------------------------ */

#define KF_IPC_HANDLE_BYTES 64
#define KF_MAX_SEGMENTS 16

/* Export the allocation holding dev_ptr for another process of this node:
 * handle[KF_IPC_HANDLE_BYTES] + the byte offset of dev_ptr inside it. */
int kf_ipc_export(const void *dev_ptr, void *handle, size_t *offset);
/* Map a peer's exported allocation; *base_out + offset is its dev_ptr. */
int kf_ipc_import(const void *handle, void **base_out);
int kf_ipc_close(void *base);
/* One launch copying nseg byte ranges dst[off_j, off_j + len_j) <-
 * srcs[j][off_j, off_j + len_j) (e.g. the shards other GPUs reduced, read
 * over xGMI); every offset, length and pointer 16-byte aligned. */
int kf_gather_segments(void *dst, const void *const *srcs, const size_t *offsets,
                       const size_t *lens, int nseg, void *stream);
/* One launch copying nseg byte ranges dsts[j][0, lens[j]) <- srcs[j][0,
 * lens[j]), any of them in a peer's HBM (the push exchange writes shards into
 * peers' buckets over xGMI); pointers and lengths 16-byte aligned. Blocks
 * alternate between segments so every link carries traffic at once. */
int kf_copy_segments(void *const *dsts, const void *const *srcs, const size_t *lens, int nseg,
                     void *stream);
/* Signal words for the device-side peer barrier: nwords zeroed 64-bit
 * words. host == 0: fine-grained, uncached device memory, exportable with
 * kf_ipc_export (every peer stores its arrival into it over xGMI); host == 1:
 * page-locked host memory the device can store into (the barrier's status
 * word, readable by the host without a sync). */
int kf_signal_alloc(size_t nwords, int host, void **ptr);
int kf_signal_free(void *ptr, int host);
/* Device-side barrier of `world` GPUs of one node, enqueued on `stream` (no
 * host round trip, no host sync): one 64-lane workgroup stores `epoch` into
 * word `rank` of every peer's signal array sigs[r] (system scope, over
 * xGMI), then waits until every word r != rank of its own array sigs[rank]
 * holds >= epoch. Stream order makes the work queued before it visible to the
 * peers (end-of-kernel release) and the work queued after it start after
 * every peer's arrival. Bounded: after timeout_us it stops waiting and stores
 * KF_ERR_TIMEOUT into status[0] (a host == 1 signal word), so a missing peer
 * cannot leave a wave spinning. epoch grows by one per barrier on every rank;
 * world <= 64. */
int kf_peer_barrier(void *const *sigs, int world, int rank, uint64_t epoch,
                    uint32_t timeout_us, void *status, void *stream);
const char *kf_p2p_last_error(void);

/* ---- pair averaging: a device-side model store (kungfu_amd/pairavg.py) ----
 *
 * What PairAveragingOptimizer (AD-PSGD, async_sgd.py) needs: every rank
 * publishes whole snapshots of its variables into slots in its own HBM; a
 * peer pulls the latest one over the pair's xGMI link and blends it into its
 * own variables. A puller gets one whole published version or nothing, never
 * a mix of two, and no kernel ever waits, spins or loops on a value another
 * rank writes.
 *
 * A plan holds, on the current device: `slots` snapshot slots (2 to 64) in
 * ONE allocation, each holding every span at a 16-byte aligned offset; a
 * control block of uncached fine-grained words (as kf_signal_alloc(.., 0)):
 * latest (versions published, 0 = none) and one seqlock per slot, odd while
 * the slot is being written; privately a staging buffer of one slot, the
 * pick record and four counters. Slots and control block are exported with
 * kf_ipc_export by the caller (kf_pairavg_local gives their addresses) and
 * every peer's mapping of them is handed back with kf_pairavg_set_peers;
 * with world == 1 the only target is the rank itself and no call is needed.
 *
 * kf_pairavg_create does all allocation. spans[i] are device pointers, 16-byte
 * aligned, of span_bytes[i] bytes (whole elements of `dt`: f32, f16, bf16 or
 * f64, else KF_ERR_DTYPE; a length may be 0; any number of spans, launched
 * KF_MAX_SEGMENTS at a time). Every rank of a group passes spans of the same
 * lengths and the same `slots`. NULL on failure, kf_pairavg_last_error()
 * starting with the status name ("KF_ERR_ARG: ...").
 *
 * Every other call only queues launches on `stream`: no allocation, no host
 * sync, safe to capture into a hipGraph (the version counter lives on the
 * device).
 *   kf_pairavg_publish        version n = published + 1 goes to slot n % slots:
 *       begin  lock[s] += 1 (odd), release store at system scope
 *       copy   variables -> slot s (16-B non-temporal; the bytes past a
 *              span's last whole vector one per lane)
 *       end    lock[s] += 1 (even), then latest = n, release stores at system
 *              scope in that order; the `published` counter becomes n
 *   kf_pairavg_pull_average   from rank `target`:
 *       pick   v0 = latest, s = v0 % slots, l0 = lock[s], acquire loads at
 *              system scope; v0 == 0: empty, l0 odd: torn
 *       fetch  the target's slot s -> staging (nothing when empty or torn)
 *       check  l1 = lock[s]; valid = (l1 == l0); exactly one of the valid /
 *              torn / empty counters grows by one
 *       blend  valid: every element v = fl_T(0.5 * fl_T(v + o)), o the staged
 *              element (TF's 0.5 * (v + other_v), async_sgd.py:130-133, in the
 *              tensor's dtype: every operation rounded to T, no contraction;
 *              f16 / bf16 compute in fp32 and round to T after the add and
 *              after the multiply). Not valid: the variables keep their bits.
 * The launch boundaries order the markers and the data. A torn pull is
 * skipped and counted, not retried: with S slots it needs the target to
 * publish twice between pick and check. The phases are also exported singly,
 * for tests and tools; the two composite calls are exactly these in order.
 * kf_pairavg_counters copies {valid, torn, empty, published} into out[4]
 * (host or device memory) with a stream-ordered asynchronous copy.
 * Slot data is ordinary device memory read by a peer: like the P2P exchange
 * it relies on the release at the writer's kernel end and the invalidate at
 * the reader's kernel start, and has only run with ranks as processes on one
 * GPU; across two physical GPUs it is unmeasured. */
#pragma GCC visibility pop
typedef struct kf_pairavg kf_pairavg_t; /* opaque plan */
#pragma GCC visibility push(default)
kf_pairavg_t *kf_pairavg_create(const void *const *spans, const size_t *span_bytes, int nspan,
                                KungFu_Datatype dt, int slots, int world, int rank);
/* This rank's slot allocation, control block and the bytes of one slot. */
int kf_pairavg_local(kf_pairavg_t *p, void **slot_base, void **ctrl_base, size_t *slot_bytes);
/* slot_bases[r] / ctrl_bases[r]: rank r's slot allocation (16-byte aligned)
 * and control block (8-byte aligned) as mapped in this process, `world`
 * entries (the plan's world); entry `rank` is ignored. */
int kf_pairavg_set_peers(kf_pairavg_t *p, const void *const *slot_bases,
                         const void *const *ctrl_bases, int world);
void kf_pairavg_destroy(kf_pairavg_t *p);
int kf_pairavg_publish(kf_pairavg_t *p, void *stream);
int kf_pairavg_pull_average(kf_pairavg_t *p, int target, void *stream);
/* the phases singly, for tests and tools */
int kf_pairavg_publish_begin(kf_pairavg_t *p, void *stream);
int kf_pairavg_publish_copy(kf_pairavg_t *p, void *stream);
int kf_pairavg_publish_end(kf_pairavg_t *p, void *stream);
int kf_pairavg_pick(kf_pairavg_t *p, int target, void *stream);
int kf_pairavg_fetch(kf_pairavg_t *p, int target, void *stream);
int kf_pairavg_check(kf_pairavg_t *p, int target, void *stream);
int kf_pairavg_blend(kf_pairavg_t *p, void *stream);
int kf_pairavg_counters(kf_pairavg_t *p, uint64_t *out /* 4 */, void *stream);
const char *kf_pairavg_last_error(void);

/* ---- multi-GPU exchange over RCCL (kungfu_amd/csrc/kf_exchange.hip) ------
 *
 * The reference's GPU collective, srcs/cpp/src/nccl/gpu_collective.cpp:
 * a communicator per process built from a unique id that rank 0 creates and
 * KungFu broadcasts (new_global, gpu_collective.cpp:190-200), then
 * ncclAllReduce per tensor with a stream sync after each call (:151-165).
 * Here the all-reduce of a bucket is split so the sum runs where the
 * north_star puts it:
 *   KF_ALGO_REDUCE_SCATTER  ncclReduceScatter -> HIP /np on the shard
 *                           (kf_bucket_div) -> in-place ncclAllGather;
 *   KF_ALGO_ALL_TO_ALL      ncclAllToAll of the shards -> HIP fold of the
 *                           world received shards IN RANK ORDER (/np fused)
 *                           -> in-place ncclAllGather. The sum is the HIP
 *                           k-input kernel, so the bits are the oracle's
 *                           reduce over ranks 0..world-1 for every dtype —
 *                           bf16 with fp32 accumulation and one rounding,
 *                           fp16 rounded per hop — equal to the P2P path;
 *                           same xGMI bytes as the reduce-scatter.
 *   KF_ALGO_REDUCE_SCATTER_AVG
 *                           for average calls: ncclReduceScatter with
 *                           ncclAvg (each input scaled by 1/world inside the
 *                           collective) -> in-place ncclAllGather, no HIP
 *                           epilogue launch. Opt-in: for f32/f64 the bits
 *                           equal KF_ALGO_REDUCE_SCATTER's (sum, then /np)
 *                           when world is a power of two and no x / world is
 *                           subnormal (scaling by 2^-k commutes with every
 *                           rounding of the sum); otherwise each input adds
 *                           one rounding. Calls without average: as
 *                           KF_ALGO_REDUCE_SCATTER.
 *   KF_ALGO_AUTO            reduce-scatter for integers and f32/f64
 *                           (RCCL's own order; integers exact; float MIN/MAX
 *                           differ from std::min/max only on NaN inputs),
 *                           all-to-all for f16/bf16 (the build's defined
 *                           semantics) and for u16/i16 (no RCCL type).
 * A count that does not split into world shards sends its last count % world
 * elements through an all-gather and the same rank-order fold. Everything
 * is queued on the caller's stream (no host sync, like RCCL); calls on one
 * exchange must be issued in the same order on every rank, and if they use
 * different streams the exchange orders its workspace between them.
 */
#define KF_UNIQUE_ID_BYTES 128
enum KF_ExchangeAlgo {
    KF_ALGO_AUTO           = 0,
    KF_ALGO_REDUCE_SCATTER = 1,
    KF_ALGO_ALL_TO_ALL     = 2,
    KF_ALGO_REDUCE_SCATTER_AVG = 3,
};
/* the reduce_scatter op a transport is asked for under
 * KF_ALGO_REDUCE_SCATTER_AVG: the sum of the inputs each scaled by 1/world
 * (ncclAvg); a transport without it returns a non-zero code */
#define KF_TRANSPORT_OP_AVG 4
#pragma GCC visibility pop
typedef struct kf_exchange kf_exchange_t; /* opaque */
#pragma GCC visibility push(default)

/* ncclGetUniqueId (rank 0 calls it, gpu_collective.cpp:196). */
int kf_exchange_unique_id(void *id);
/* Broadcast rank 0's id[KF_UNIQUE_ID_BYTES] to every peer of a session, in
 * place (Peer::Broadcast of the id, gpu_collective.cpp:197-198). */
int kf_exchange_share_id(kf_session_t *s, void *id);
/* ncclCommInitRank on HIP device `device` (the caller's current device is
 * restored). NULL on failure (kf_exchange_last_error). */
kf_exchange_t *kf_exchange_create(const void *id, int rank, int world, int device);
/* kf_exchange_create that gives up after timeout_ms (< 0: wait as long as it
 * takes) with KF_ERR_TIMEOUT in kf_exchange_last_error, when not every rank
 * joined the communicator's init in time. The init it abandons keeps waiting
 * on a helper thread (a late completion releases its communicator). */
kf_exchange_t *kf_exchange_create_timeout(const void *id, int rank, int world, int device,
                                          int timeout_ms);
/* gpu_collective::new_global: id from rank 0, shared over the session, then
 * kf_exchange_create(id, rank, size, device). */
kf_exchange_t *kf_exchange_create_session(kf_session_t *s, int rank, int world, int device);
/* recv = all-reduce(send) (op; average != 0: SUM then / world, float types).
 * send == recv is in place. */
int kf_exchange_all_reduce(kf_exchange_t *ex, const void *send, void *recv, size_t count,
                           KungFu_Datatype dt, KungFu_Op op, int average, int algo,
                           void *stream);
/* nb buckets in one call, each reduced as by kf_exchange_all_reduce: one
 * grouped RCCL launch per phase and one batched HIP launch
 * (kf_bucket_reduce_batch) for all shard epilogues / folds. */
int kf_exchange_all_reduce_batch(kf_exchange_t *ex, const void *const *sends, void *const *recvs,
                                 const size_t *counts, int nb, KungFu_Datatype dt, KungFu_Op op,
                                 int average, int algo, void *stream);
/* SMA (sma_sgd.py:60-65) for nb variable buckets: sums[b] = all-reduce-sum of
 * vs[b], then vs[b] = (1 - alpha) vs[b] + alpha sums[b] / world
 * (kf_sma_blend). sums[b] are caller workspaces of counts[b] elements. */
int kf_exchange_sma_batch(kf_exchange_t *ex, void *const *vs, void *const *sums,
                          const size_t *counts, int nb, KungFu_Datatype dt, double alpha,
                          int algo, void *stream);
/* The synchronous step with the optimizer update on the shard (sharded
 * optimizer state): reduce-scatter of the gradient buckets, kf_sgd_update_batch
 * on this rank's shard of every bucket (params[b] + rank * q, grads[b] +
 * rank * q, mom_shards[b], q = counts[b] / world elements), in-place all-gather
 * of the PARAMETER buckets. Reduce-scatter: the shard holds the sum and the
 * update divides by world. All-to-all (f16 / bf16 under KF_ALGO_AUTO): the
 * rank-order fold applies the / world and the update divides by nothing.
 * KF_ALGO_REDUCE_SCATTER_AVG: the / world inside the collective. World 1 on
 * the built-in transport is the update over the whole buckets.
 * counts[b] is a multiple of world and every shard starts 16-byte aligned
 * (no tails); mom_shards[b] holds q elements, and may be NULL where
 * hyper[b].momentum == 0. After the call the gradient buckets hold nothing
 * defined: they are scratch of the call. Follows kf_exchange_set_timing (the
 * update counts under phase 2, the parameters' all-gather under phase 3) and
 * always runs un-pipelined. */
int kf_exchange_sgd_batch(kf_exchange_t *ex, void *const *params, void *const *grads,
                          void *const *mom_shards, const size_t *counts, int nb,
                          KungFu_Datatype dt, const kf_sgd_hyper *hyper, int algo, void *stream);
/* kf_exchange_sgd_batch with the Adam / AdamW update (kf_adam_update_batch)
 * on the shard: reduce-scatter of the gradient buckets (under auto, bf16
 * takes the all-to-all and the rank-order fold), the update on params[b] +
 * rank * q, grads[b] + rank * q, exp_avg_shards[b] and exp_avg_sq_shards[b]
 * of q = counts[b] / world elements (np = world after a plain reduce-scatter,
 * 0 after the fold or under rs_avg), in-place all-gather of the PARAMETER
 * buckets. World 1 on the built-in transport runs the update over the whole
 * buckets with np = 1. f32, f64 and bf16. Every counts[b] is a multiple of
 * the world, buckets and shards start 16-byte aligned and both state shards
 * are there for every non-empty bucket, or KF_ERR_ARG before any collective.
 * hyper[b].lr etc. as kf_adam_update_batch. Un-pipelined; follows
 * kf_exchange_set_timing as kf_exchange_sgd_batch does. */
int kf_exchange_adam_batch(kf_exchange_t *ex, void *const *params, void *const *grads,
                           void *const *exp_avg_shards, void *const *exp_avg_sq_shards,
                           const size_t *counts, int nb, KungFu_Datatype dt,
                           const kf_adam_hyper *hyper, int algo, void *stream);
/* kf_exchange_adam_batch for 16-bit parameter and gradient buckets (dt bf16 or
 * f16, KF_ERR_DTYPE otherwise) with fp32 master weights and state
 * (kf_adam_master_update_batch) on the shard: phases 1 and 3 are the Adam
 * call's on the 16-bit buckets; phase 2 runs on params[b] + rank * q, the
 * received gradient shard, and master_shards[b], exp_avg_shards[b] and
 * exp_avg_sq_shards[b] of q = counts[b] / world fp32 elements. The same
 * up-front checks on every rank, and the master shard must be there for every
 * non-empty bucket. World 1 on the built-in transport runs the update over
 * the whole buckets with np = 1. Un-pipelined; follows kf_exchange_set_timing. */
int kf_exchange_adam_master_batch(kf_exchange_t *ex, void *const *params, void *const *grads,
                                  void *const *master_shards, void *const *exp_avg_shards,
                                  void *const *exp_avg_sq_shards, const size_t *counts, int nb,
                                  KungFu_Datatype dt, const kf_adam_hyper *hyper, int algo,
                                  void *stream);
/* The gated step (kf_step_gate_update above) is
 * kf_exchange_adam_batch / kf_exchange_adam_master_batch split in two, with
 * the verdict over ALL of an optimizer's bucket groups between the halves:
 *   A  kf_exchange_reduce_shards_batch per group: phase 1 and the rank-order
 *      folds. This rank's reduced shard of bucket b is left at grads[b] +
 *      rank * q (q = counts[b] / world), and *np is what the update must
 *      still divide by: the world after a plain reduce-scatter, 0 after the
 *      fold or under rs_avg. World 1 on the built-in transport does nothing
 *      and reports 1 (the whole buckets are the shards).
 *   B  kf_segnorm_run over the shards, C  kf_exchange_all_gather_doubles,
 *   D  kf_step_gate_update
 *   E  kf_exchange_adam_gated_batch per group: kf_adam_update_batch_gated
 *      (master_shards == NULL; f32, f64, bf16) or
 *      kf_adam_master_update_batch_gated (bf16, f16) on the shards with np as
 *      step A reported it, then phase 3, the parameters' in-place all-gather.
 *      One hyper for the whole call, its bias corrections ignored; gate and
 *      state are device pointers.
 * Both halves make kf_exchange_adam_batch's up-front checks (multiples of the
 * world, 16-byte alignment, every shard present) on every rank before any
 * collective. Everything is queued on `stream`; un-pipelined; both follow
 * kf_exchange_set_timing (A counts under phases 1 and 2, E under 2 and 3). */
int kf_exchange_reduce_shards_batch(kf_exchange_t *ex, void *const *grads, const size_t *counts,
                                    int nb, KungFu_Datatype dt, int algo, int *np, void *stream);
int kf_exchange_adam_gated_batch(kf_exchange_t *ex, void *const *params, void *const *grads,
                                 void *const *master_shards, void *const *exp_avg_shards,
                                 void *const *exp_avg_sq_shards, const size_t *counts, int nb,
                                 KungFu_Datatype dt, int np, const kf_adam_hyper *hyper,
                                 const kf_step_gate *gate, const kf_step_state *state, void *stream);
/* recv[r * n + k] = rank r's send[k], k < n: the transport's byte all_gather
 * of n doubles per rank (device pointers; send may be recv + rank * n). World
 * 1 on the built-in transport is a copy. */
int kf_exchange_all_gather_doubles(kf_exchange_t *ex, const double *send, double *recv, int n,
                                   void *stream);
/* Phase 3 alone: the in-place all-gather of the parameter buckets, params[b] +
 * rank * q (q = counts[b] / world elements) to every rank, for a step whose
 * update ran outside the exchange (LAMB). It makes
 * kf_exchange_adam_batch's up-front checks on every rank before any
 * collective: a float dtype, every counts[b] a multiple of the world, buckets
 * and shards 16-byte aligned. World 1 on the built-in transport does nothing.
 * Queued on `stream`; un-pipelined; follows kf_exchange_set_timing under
 * phase 3. */
int kf_exchange_gather_params_batch(kf_exchange_t *ex, void *const *params, const size_t *counts,
                                    int nb, KungFu_Datatype dt, void *stream);
/* Pipelined schedule for the batch calls (default 1 = off): the buckets of a
 * call are split into `groups` groups of consecutive buckets of about equal
 * bytes; the RCCL phases stay on the caller's stream in the same order on
 * every rank (group g+1's reduce-scatter / all-to-all before group g's
 * all-gather), and the element-wise work of group g (its shard epilogue or
 * rank-order fold, and for SMA its blends) runs on the exchange's own stream
 * meanwhile, ordered by events. Same results bit for bit. */
int kf_exchange_set_pipeline(kf_exchange_t *ex, int groups);
/* Opt-in per-phase timing of the batch calls (kf_exchange_all_reduce,
 * kf_exchange_all_reduce_batch, kf_exchange_sma_batch, kf_exchange_sgd_batch)
 * on the un-pipelined schedule: timing events on the caller's stream before phase 1 (every
 * bucket's reduce-scatter or all-to-all, and the tail gathers), phase 2 (the
 * /np epilogue or rank-order fold), phase 3 (the all-gathers), the SMA blend,
 * and after it. on != 0 starts a window with zeroed sums, 0 ends it. Costs
 * five event records per call; off by default. */
int kf_exchange_set_timing(kf_exchange_t *ex, int on);
/* The window's sums in microseconds: us[0] phase 1, us[1] phase 2, us[2]
 * phase 3, us[3] blend; *calls the timed calls, *untimed the pipelined ones
 * (their phases overlap on two streams, so they are not split). Waits for the
 * timed calls queued so far. calls / untimed may be NULL. */
int kf_exchange_phase_times(kf_exchange_t *ex, double *us, int64_t *calls, int64_t *untimed);
/* Ordered issue of concurrently produced all-reduces, the reference's
 * NCCLScheduler / LinearExecutor (srcs/cpp/src/nccl/scheduler.cpp:8-130):
 * begin_step fixes this step's names in an order every rank shares;
 * kf_exchange_start may be called for them in any order from any thread, and
 * the exchange's thread issues them strictly in that order (a name waits for
 * every name before it). With auto_order, the second step adopts rank 0's
 * arrival order of the first (broadcast over the communicator, as
 * NCCLScheduler::Reset does with Peer::Broadcast). done(status, arg) runs
 * when that all-reduce has completed on the device. */
int kf_exchange_begin_step(kf_exchange_t *ex, const char *const *names, int n, int auto_order);
int kf_exchange_start(kf_exchange_t *ex, const char *name, const void *send, void *recv,
                      size_t count, KungFu_Datatype dt, KungFu_Op op, int average, int algo,
                      void *stream, kf_done_fn done, void *arg);
/* Wait until every started all-reduce of the step has completed; the first
 * failure (its message in kf_exchange_last_error on this thread), else KF_OK.
 * *order (if not NULL, n entries) receives the issue order used. Destroy an
 * exchange only after this returned: tasks still queued are not issued and
 * their done callbacks never run. */
int kf_exchange_wait_all(kf_exchange_t *ex, int32_t *order);
/* KF_OK, or KF_ERR_RCCL after an asynchronous RCCL failure
 * (ncclCommGetAsyncError). */
int kf_exchange_check(kf_exchange_t *ex);
int kf_exchange_info(kf_exchange_t *ex, int *rank, int *world, int *device);
/* What the transport itself reports, for the bench line and logs: the RCCL
 * communicator's rank count (ncclCommCount) and RCCL's version
 * (ncclGetVersion, e.g. 22703). -1 / 0 for a host's own transport
 * (kf_exchange_create_transport) or a librccl without the symbol. A count
 * other than the exchange's world means the ranks did not form one
 * communicator. (The reference's nccl path asks neither,
 * srcs/cpp/src/nccl/gpu_collective.cpp:151-165; diagnostic only.) */
int kf_exchange_transport_info(kf_exchange_t *ex, int *comm_count, int *rccl_version);
void kf_exchange_destroy(kf_exchange_t *ex);
const char *kf_exchange_last_error(void);

/* Name-keyed all-reduce: GoKungfuAllReduce(send, recv, count, dtype, op,
 * name, done) (srcs/go/libkungfu-comm/collective.go:34-45) on the exchange.
 * Each rank may start its names in ANY order, from any thread: tensors pair
 * by name across ranks, as the reference's per-name mailbox pairs messages
 * (srcs/go/rchannel/handler/collective.go:48-64), not by call order. An
 * exchange thread agrees the issue order with the peers in negotiation
 * cycles (one all-gather of the newly started names per cycle over a second
 * communicator split off at the first call, so negotiating never waits
 * behind queued data collectives); a name is issued once every rank started
 * it, in rank 0's start order, and names that become ready in one cycle with
 * the same dtype / op / average / algo go out as ONE batched call (grouped
 * RCCL phases, one HIP launch). The data moves on the exchange's own stream
 * after the work queued on `stream` before this call; done(status, arg)
 * runs once the all-reduce finished on the device (kf_exchange_last_error
 * inside done gives a failure's message). A name may be outstanding once per
 * rank; count, dtype, op and average must agree across ranks (a mismatch
 * fails that name with KF_ERR_ARG on every rank). An empty name is the
 * anonymous call of a blocking op (the reference's all_reduce_cuda): the
 * exchange names it from its own counter, so such calls pair across ranks by
 * their order on each rank's exchange. Do not interleave these with the
 * ordered calls above on one exchange. */
int kf_exchange_all_reduce_named(kf_exchange_t *ex, const char *name, const void *send, void *recv,
                                 size_t count, KungFu_Datatype dt, KungFu_Op op, int average,
                                 int algo, void *stream, kf_done_fn done, void *arg);
/* Block until every name started so far on this rank has completed; the
 * first failure since the previous wait (message in kf_exchange_last_error),
 * else KF_OK. Destroy an exchange only after this returned. */
int kf_exchange_wait_named(kf_exchange_t *ex);

/* ---- exchange transports ---------------------------------------------------
 * The exchange issues five collectives and moves every byte through them; a
 * transport is the table of those collectives bound to one communicator.
 * kf_exchange_create binds the built-in librccl transport (RCCL over xGMI).
 * kf_exchange_create_transport binds any other one — a host's own collective
 * library, or a stand-in that lets the exchange's multi-rank logic run where
 * RCCL cannot (several ranks on one device; tests/c/kf_testing.cpp). Every
 * function queues its work on `stream` (a hipStream_t) in call order and
 * returns 0, or a transport code that error_string explains. The calls
 * between group_start and group_end belong to one phase and may be fused.
 * reduce_scatter sums count elements per rank (op, dt as the exchange's own
 * kernels define them, or KF_TRANSPORT_OP_AVG) and may refuse a dtype or op
 * with a non-zero code; the
 * AUTO algo never asks for an f16 / bf16 / u16 / i16 reduce-scatter. split
 * (ncclCommSplit's contract: collective over comm; ranks of one color form a
 * communicator ordered by key) is needed by kf_exchange_split and the named
 * all-reduce. The table must outlive every exchange bound to it; the
 * exchange owns `comm` and releases it with destroy. */
typedef struct kf_transport_ops {
    int (*group_start)(void *comm);
    int (*group_end)(void *comm);
    int (*reduce_scatter)(const void *send, void *recv, size_t count, KungFu_Datatype dt,
                          KungFu_Op op, void *comm, void *stream);
    int (*all_gather)(const void *send, void *recv, size_t bytes, void *comm, void *stream);
    int (*all_to_all)(const void *send, void *recv, size_t bytes, void *comm, void *stream);
    int (*broadcast)(const void *send, void *recv, size_t bytes, int root, void *comm,
                     void *stream);
    int (*split)(void *comm, int color, int key, void **newcomm);
    int (*async_error)(void *comm);
    void (*destroy)(void *comm);
    const char *(*error_string)(int code);
} kf_transport_ops;
/* An exchange of rank `rank` of `world` on HIP device `device` over `ops`
 * bound to `comm` (ownership passes to the exchange; on failure the caller
 * keeps it). A one-rank exchange over a transport still calls it (only the
 * built-in RCCL transport short-cuts world 1 to a copy). */
kf_exchange_t *kf_exchange_create_transport(const kf_transport_ops *ops, void *comm, int rank,
                                            int world, int device);
/* gpu_collective::new_local / new_group (srcs/cpp/src/nccl/gpu_collective.cpp:
 * 202-243): a new exchange over the ranks of `ex` that pass the same color,
 * ranked by key (ties by rank), on the same device. Collective over `ex`:
 * every rank calls it at the same point of its call sequence. color < 0:
 * this rank joins none (returns NULL with KF_OK in *status). The local scope
 * is color = host index, key = rank (kf_exchange_create_local). */
kf_exchange_t *kf_exchange_split(kf_exchange_t *ex, int color, int key, int *status);

/* ---- hierarchical all-reduce (several hosts, several GPUs each) -----------
 * gpu_collective::new_local (srcs/cpp/src/nccl/gpu_collective.cpp:202-212):
 * an exchange over this host's ranks of the session `s` (same IPv4), ranked
 * in the session's order. Each host's first rank creates the RCCL id; every
 * host's id travels in ONE session all-reduce of hosts x 128 bytes (one
 * contributor per slot, so the sum is the id). Collective over `s`. */
kf_exchange_t *kf_exchange_create_local(kf_session_t *s, int device);
/* ScheduledHierarchicalNcclAllReduce (srcs/cpp/src/tensorflow/ops/gpu/
 * collective.cpp:108-162: ncclReduce in the host -> CrossAllReduceGpu over
 * the hosts, nccl/controller.cpp:7-39 -> ncclBroadcast in the host), with the
 * bucket sharded across the host's GPUs when every host has as many:
 *   1. local reduce-scatter (algo: RCCL's, or the all-to-all + HIP rank-order
 *      fold) — local rank j holds shard j of its host's sum;
 *   2. the shard all-reduced across hosts by the device-mode session `cross`
 *      among the ranks with the same local rank (kf_session_subset_all_reduce,
 *      one tree per local rank), so every link carries 1/local_size of it;
 *   3. average: / size() on the shard (kf_bucket_div);
 *   4. local in-place all-gather.
 * Hosts of different sizes take the reference's path: local all-reduce, the
 * hosts' first ranks all-reduce across hosts, local broadcast. `local` must
 * hold exactly this host's ranks in session order (kf_exchange_create_local,
 * or any transport with that layout); every rank calls with the same name,
 * count, dtype and op, in the same order. Buffers are HBM; queued on
 * `stream`, blocking on the host while the cross-host step runs. */
int kf_hier_all_reduce(kf_exchange_t *local, kf_session_t *cross, const void *send, void *recv,
                       size_t count, KungFu_Datatype dt, KungFu_Op op, int average, int algo,
                       const char *name, void *stream);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
