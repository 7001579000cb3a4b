// pcb_policy_eval.hip -- k_evaluate_logits and k_evaluate_logits_backward: log-probability and entropy of stored
// actions under a policy's masked categorical, and their gradient with respect to the logits
// (pcbenv_evaluate_logits, pcbenv_evaluate_logits_backward).  Part of libpcbenv.so (CDNA4 / gfx950 only); a translation
// unit of its own, so that nothing here can change the builds of k_step / k_reset / k_gather / k_sample / k_sample_logits.
//
// This is the update half of the reference's masked Categorical (RLlib's Categorical.logp / entropy of
// `logits += max(log(action_mask), float32.min)`, utils/agent/factorized_action_distributions.py:21-91): what a PPO
// update evaluates for every minibatch.  The rows are stored steps, not the handle's environments: the legal set of a
// row comes from the caller's bit rows ([num_rows, 2, H, WW], the layout of pcbenv_mask_bits), and a logit is read only
// where its action is legal, as in k_sample_logits.
//
// One workgroup per row (xcd_contiguous_env: each XCD streams a contiguous share of the logits and of the gradient),
// four wavefronts when A = O*H*W >= 4096, otherwise one.  Segments (the up to 64 logits one mask word governs), the
// chunk loads, pass 1, the legal count and the combine's per-lane partials are those of k_sample_logits
// (pcb_policy_common.h).
//   forward   per segment (m = max, s = sum exp(l - m), t = sum exp(l - m) (l - m)) -> LDS; wavefront 0 combines them
//             in float64 (M, Z, sum p (l - M)) and counts the legal bits; the stored action's logit is read directly and
//             its bit checked.  (M, log Z, entropy, row status) go to `stats` for the backward kernel.
//   backward  one pass: a chunk of 4 with no legal bit stores zeros without loading; otherwise
//             p = exp2((l - M - log Z) log2 e), g = g_lp (1[i = a] - p) - g_H p (log p + Hrow), whole vectors stored.
#include <hip/hip_runtime.h>

#include "pcbenv.h"
#include "pcb_launch.h"
#include "pcb_policy_common.h"

namespace {

// Segments per lane whose loads are issued before the first is used (as PCB_SL_UNROLL), and the smallest A launched with
// four wavefronts.  -DPCB_EV_NT_STORES: the gradient is written with non-temporal stores (store_vec in
// pcb_policy_common.h; A/B builds only; profiles/evaluate_logits_ab.txt).
#ifndef PCB_EV_UNROLL
#define PCB_EV_UNROLL 4
#endif
#ifndef PCB_EV_NW4_MIN_A
#define PCB_EV_NW4_MIN_A 4096
#endif
constexpr int UNROLL = PCB_EV_UNROLL;

// row status in stats[4 r + 3]
constexpr float ROW_OK = 0.f, ROW_ZERO = 1.f, ROW_NO_ONE_HOT = 2.f;

template <typename T, bool VEC, int NW>
__global__ __launch_bounds__(64 * NW) void k_evaluate_logits(EvalGeom q, EvalLogitsArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = xcd_contiguous_env((int)blockIdx.x, 0, q.rows), tid = threadIdx.x, lane = tid & (WAVE - 1);
    const PolicyLds lds = carve_lds(smem, q);
    stage_bits(lds.vml, g.mask_bits + (size_t)e * (size_t)(2 * q.H * q.WW), q, tid, 64 * NW);
    if (tid == 0) *lds.bad = 0;
    __syncthreads();

    const T *row = (const T *)g.logits + (size_t)e * (size_t)(q.O * q.H * q.W);
    // the stored action's logit, in flight under pass 1
    bool a_legal = false;
    int a = -1;
    float la = 0.f;
    if (tid == 0) {
        a = stored_action(lds.vml, q, g.actions, g.fmt, e, &a_legal);
        if (a_legal) la = to_f32(row[a]);
    }
    if (pass1<T, VEC, NW, UNROLL, false>(row, lds, q, tid, false)) *lds.bad = 1;
    __syncthreads();
    if (tid >= WAVE) return;

    // ---- wavefront 0: the legal count, M, Z, the outputs
    int j0, j1;
    lane_run(q.O * q.H * q.WW, lane, &j0, &j1);
    const auto [n, M, bad_bits] = row_head(lds, q, j0, j1, lane);
    double mine = 0.0, tl = 0.0;
    if (n > 0 && !bad_bits) combine_partials(lds, j0, j1, M, &mine, &tl);
    const double Z = wave_sum(mine), tsum = wave_sum(tl);
    if (lane != 0) return;
    unsigned bits = bad_bits;
    float status = ROW_ZERO, statM = 0.f, statLogZ = 0.f;
    double logp = 0.0, ent = 0.0;
    if (n > 0 && bad_bits) {
        logp = -log((double)n); ent = log((double)n);
    } else if (n > 0) {
        const double logZ = log(Z);
        ent = logZ - tsum / Z;
        statM = M; statLogZ = (float)logZ;
        if (a_legal) { logp = (double)la - (double)M - logZ; status = ROW_OK; }
        else { bits |= 4u; status = ROW_NO_ONE_HOT; }
    }
    if (g.log_prob) g.log_prob[e] = (float)logp;
    if (g.entropy) g.entropy[e] = (float)ent;
    if (g.stats) {
        float4 st;
        st.x = statM; st.y = statLogZ; st.z = (float)ent; st.w = status;
        *(float4 *)(g.stats + 4 * (size_t)e) = st;
    }
    if (bits && g.errors) atomicOr(g.errors, bits);
}

template <typename T, bool VEC, int NW>
__global__ __launch_bounds__(64 * NW) void k_evaluate_logits_backward(EvalGeom q, EvalLogitsBackwardArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = xcd_contiguous_env((int)blockIdx.x, 0, q.rows), tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int S = q.O * q.H * q.WW;
    u64 *vml = (u64 *)smem;
    stage_bits(vml, g.mask_bits + (size_t)e * (size_t)(2 * q.H * q.WW), q, tid, 64 * NW);
    const float4 st = *(const float4 *)(g.stats + 4 * (size_t)e);
    const float M = st.x, logZ = st.y, Hrow = st.z;
    const bool zero_row = st.w == ROW_ZERO;
    const float glp = g.grad_log_prob ? g.grad_log_prob[e] : 0.f, gH = g.grad_entropy ? g.grad_entropy[e] : 0.f;
    __syncthreads();
    int a = -1;
    if (st.w == ROW_OK) {  // the forward call found the action in range and legal
        bool legal;
        a = stored_action(vml, q, g.actions, g.fmt, e, &legal);
    }
    const size_t base = (size_t)e * (size_t)(q.O * q.H * q.W);
    const T *row = (const T *)g.logits + base;
    T *out = (T *)g.grad_logits + base;
    const int sub = lane & (SEG_LANES - 1), grp = tid >> 4;
    constexpr int G = 64 * NW / SEG_LANES;
    for (int s0 = 0; s0 < S; s0 += G * UNROLL) {
        float v[UNROLL][4];
        unsigned nib[UNROLL];
        int a0[UNROLL], cols[UNROLL];  // cols: how many of this lane's 4 columns exist (all of them get a gradient)
        #pragma unroll
        for (int u = 0; u < UNROLL; u++) nib[u] = load_chunk<T, VEC>(row, vml, q, s0 + u * G + grp, S, sub, zero_row, v[u], &a0[u], &cols[u]);
        #pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            float gr[4];
            #pragma unroll
            for (int i = 0; i < 4; i++)
                gr[i] = ((nib[u] >> i) & 1u) ? grad_one(v[u][i], M, logZ, Hrow, glp, gH, a0[u] + i == a) : 0.f;
            if (VEC) {
                if (cols[u]) store4(out + a0[u], gr);
            } else {
                #pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < cols[u]) store1(out + a0[u] + i, gr[i]);
            }
        }
    }
}

}  // namespace

int pcb_launch_evaluate_logits(const EvalLogitsLaunch &a) {
    const EvalGeom &q = a.q;
    select_launch(a.dtype, q.W, (uintptr_t)a.g.logits, q.O * q.H * q.W, PCB_EV_NW4_MIN_A, [&](auto t, auto vec, auto nw) {
        hipLaunchKernelGGL((k_evaluate_logits<typename decltype(t)::type, vec, nw>), dim3(q.rows), dim3(64 * nw), lds_bytes(q), a.stream, q, a.g);
    });
    return 0;
}

// the gradient is stored with the same vectors as the logits are loaded: both pointers aligned; LDS: the bit rows alone
int pcb_launch_evaluate_logits_backward(const EvalLogitsBackwardLaunch &a) {
    const EvalGeom &q = a.q;
    const uintptr_t both = (uintptr_t)a.g.logits | (uintptr_t)a.g.grad_logits;
    select_launch(a.dtype, q.W, both, q.O * q.H * q.W, PCB_EV_NW4_MIN_A, [&](auto t, auto vec, auto nw) {
        hipLaunchKernelGGL((k_evaluate_logits_backward<typename decltype(t)::type, vec, nw>), dim3(q.rows), dim3(64 * nw),
                           (size_t)16 * q.H * q.WW, a.stream, q, a.g);
    });
    return 0;
}
