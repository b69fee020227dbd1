// kf_step_gate.hip — the verdict of a gated optimizer step (include/kungfu_amd.h
// kf_step_gate_update): from the ranks' sums of squares of
// their gradient shards to skip / grad_mul, the loss scale's update and every
// parameter group's step count and bias-correction scalars, on the device, so
// that a step with gradient clipping, loss scaling and inf / NaN skipping
// needs no host sync. kf_noise_scale_update's shape (kf_segnorm.hip): one
// working lane, fp64 with one IEEE operation per intrinsic, no contraction, no
// atomics. The gated update kernels (kf_adam.hip, kf_adam_master.hip) read
// what this writes.
//
// One launch holds kGatePlans plans' np and kGateGroups groups' scalars in its
// kernel arguments; a longer list takes more launches on the same stream, the
// running total kept in the gate between them. The plans come first, the
// verdict with the last of them, the groups after it.
#include <hip/hip_runtime.h>

#include <string>

#include "kf_update_batch.hpp"  // UpdateFail, launch_status

namespace kf
{
constexpr int kGatePlans  = 64;
constexpr int kGateGroups = 16;

struct GateArgs {
    int np[kGatePlans];
    kf_step_group grp[kGateGroups];
    int k0, nk;         // this launch's plans: k0 .. k0 + nk of nplan
    int first, verdict; // zero the total before; decide after
    int ng;             // this launch's groups: states[0 .. ng)
};
struct GateRule {
    double max_norm;
    float growth, backoff;
    int interval;
};
static_assert(sizeof(GateArgs) + sizeof(GateRule) + 64 <= 3072, "kernarg budget");

__global__ void step_gate_kernel(GateArgs a, GateRule rule, const double *__restrict__ sq,
                                 int world, int nplan, kf_step_state *__restrict__ states,
                                 kf_step_gate *__restrict__ gate)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (a.nk > 0 || a.first) {
        double total = a.first ? 0.0 : gate->total;
        for (int i = 0; i < a.nk; ++i) {
            const int k = a.k0 + i;
            double s    = 0.0;
            for (int r = 0; r < world; ++r) {
                s = __dadd_rn(s, sq[static_cast<size_t>(r) * nplan + k]);
            }
            if (a.np[i] > 0) {
                const double n = static_cast<double>(a.np[i]);
                s              = __ddiv_rn(s, __dmul_rn(n, n));
            }
            total = __dadd_rn(total, s);
        }
        gate->total = total;
    }
    if (a.verdict) {
        const double total = gate->total;
        const bool skip    = !(fabs(total) < __builtin_huge_val());  // inf or NaN
        const float scale  = gate->loss_scale;
        const double ls    = static_cast<double>(scale);
        const double norm  = __ddiv_rn(__dsqrt_rn(total), ls);
        double clip        = 1.0;
        if (rule.max_norm > 0) {
            const double x = __ddiv_rn(rule.max_norm, __dadd_rn(norm, 1e-6));
            if (x < 1.0) clip = x;
        }
        gate->skip      = skip ? 1 : 0;
        gate->grad_norm = norm;
        gate->grad_mul  = static_cast<float>(__ddiv_rn(clip, ls));
        // torch.amp.GradScaler's update (_amp_update_scale_), fp32
        if (skip) {
            gate->loss_scale = __fmul_rn(scale, rule.backoff);
            gate->good_steps = 0;
            gate->skipped += 1;
        } else {
            const int good = gate->good_steps + 1;
            if (good == rule.interval) {
                const float grown = __fmul_rn(scale, rule.growth);
                if (fabsf(grown) < __builtin_huge_valf()) gate->loss_scale = grown;
                gate->good_steps = 0;
            } else {
                gate->good_steps = good;
            }
            gate->applied += 1;
        }
    }
    if (a.ng > 0 && gate->skip == 0) {
        for (int j = 0; j < a.ng; ++j) {
            const kf_step_group &g = a.grp[j];
            kf_step_state &st      = states[j];
            const double b1p       = __dmul_rn(st.beta1_pow, g.beta1);
            const double b2p       = __dmul_rn(st.beta2_pow, g.beta2);
            const double s2        = __dsqrt_rn(__dsub_rn(1.0, b2p));
            const double nss       = -__ddiv_rn(g.lr, __dsub_rn(1.0, b1p));
            st.beta1_pow           = b1p;
            st.beta2_pow           = b2p;
            st.step += 1;
            st.s2_f64  = s2;
            st.nss_f64 = nss;
            st.s2      = static_cast<float>(s2);
            st.nss     = static_cast<float>(nss);
        }
    }
}

}  // namespace kf

namespace
{
using namespace kf;
constexpr UpdateFail fail{"kf_step_gate_update"};
}  // namespace

extern "C" {

int kf_step_gate_update(const double *sq, int world, int nplan, const int *np,
                        const kf_step_group *groups, kf_step_state *states, int ngroup,
                        double max_norm, double growth_factor, double backoff_factor,
                        int growth_interval, kf_step_gate *gate, void *stream)
{
    if (!sq || !np || !gate) return fail(KF_ERR_ARG, "KF_ERR_ARG", "null pointer");
    if (world < 1 || nplan < 1) return fail(KF_ERR_ARG, "KF_ERR_ARG", "world and nplan must be >= 1");
    if (ngroup < 0 || (ngroup > 0 && (!groups || !states))) {
        return fail(KF_ERR_ARG, "KF_ERR_ARG", "ngroup < 0, or groups without their tables");
    }
    if (growth_interval < 0) return fail(KF_ERR_ARG, "KF_ERR_ARG", "growth_interval < 0");
    if (!(growth_factor > 0) || !(backoff_factor > 0)) {
        return fail(KF_ERR_ARG, "KF_ERR_ARG", "growth and backoff factors must be > 0");
    }
    for (int k = 0; k < nplan; ++k) {
        if (np[k] < 0) return fail(KF_ERR_ARG, "KF_ERR_ARG", "np < 0");
    }
    const GateRule rule{max_norm, static_cast<float>(growth_factor),
                        static_cast<float>(backoff_factor), growth_interval};
    hipStream_t s = static_cast<hipStream_t>(stream);
    int k = 0, g = 0;
    bool decided = false;
    while (!decided || g < ngroup) {
        GateArgs a;
        a.k0    = k;
        a.first = k == 0 && !decided;
        a.nk    = decided ? 0 : (nplan - k < kGatePlans ? nplan - k : kGatePlans);
        for (int i = 0; i < kGatePlans; ++i) a.np[i] = i < a.nk ? np[k + i] : 0;
        k += a.nk;
        a.verdict = !decided && k == nplan;
        if (a.verdict) decided = true;
        // the groups follow the verdict: from its own launch on
        a.ng = decided ? (ngroup - g < kGateGroups ? ngroup - g : kGateGroups) : 0;
        for (int j = 0; j < kGateGroups; ++j) {
            a.grp[j] = j < a.ng ? groups[g + j] : kf_step_group{0.0, 0.0, 0.0};
        }
        step_gate_kernel<<<1, 64, 0, s>>>(a, rule, sq, world, nplan, states ? states + g : nullptr,
                                          gate);
        const int rc = launch_status(fail);
        if (rc != KF_OK) return rc;
        g += a.ng;
    }
    return KF_OK;
}

}  // extern "C"
