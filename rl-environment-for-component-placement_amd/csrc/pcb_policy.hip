// pcb_policy.hip -- k_sample_logits: a policy's masked categorical draw from its logits (pcbenv_sample_logits).
// Part of libpcbenv.so (CDNA4 / gfx950 only); a translation unit of its own, so that nothing here can change the
// builds of k_step / k_reset / k_gather / k_sample.
//
// The reference's models mask their logits (`logits += max(log(action_mask), float32.min)`,
// agent/models/square_model.py:137-139) and hand them to RLlib's Categorical
// (utils/agent/factorized_action_distributions.py:21-91): sample / deterministic_sample, logp, entropy.  Here the legal
// set is read from the state block's bit rows instead of the uint8 action_mask, and a logit is read only where its
// action is legal: a 16-byte chunk with no legal bit issues no load, so the cache lines of an occupied board are never
// fetched.
//
// One workgroup per environment (xcd_contiguous_env: each XCD streams a contiguous share of the logits), four
// wavefronts when A = O*H*W >= 4096, otherwise one.
//   segment   (o, x, 64-column word w): the up to 64 logits one mask word governs, flat [(o*H + x)*W + 64 w, + len).
//             There are O*H*WW of them (c3 256, c5 1024).
//   pass 1    a 16-lane DPP row per segment, 4 logits per lane, U segments' loads in flight per lane before the first
//             use; per segment (m = max, s = sum exp(l - m), t = sum exp(l - m) (l - m), first index of the max) -> LDS.
//   pick      wavefront 0 combines the segments in float64 (M, Z, the prefix, sum p (l - M)), finds the segment J that
//             holds u*Z, re-reads J (<= 256 bytes, just fetched) and selects the element; one lane writes the results.
// Pass 1, the chunk loads, the legal count and the combine's per-lane partials are those of k_evaluate_logits
// (pcb_policy_common.h); the scan that gives the prefix and Z, and the pick, are this kernel's own.
// Weights are exp2((l - m) * log2 e) in float32, computed by one function in both passes, so the re-read of J sees
// exactly the weights its sum was made of.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "pcbenv.h"
#include "pcb_sampler.h"
#include "pcb_launch.h"
#include "pcb_policy_common.h"
#include "pcb_transition.h"

namespace {

// Segments per lane whose loads are issued before the first is used, and the smallest A launched with four wavefronts.
// (-D overrides for A/B builds only: c3 x 4096 fp32 measured 67 us with 4 / four wavefronts -- 60 VGPRs, 8 waves per
// SIMD -- against 79 us with 8 (103 VGPRs, 4 waves per SIMD) and 77 us with one wavefront per environment;
// profiles/sample_logits_ab.txt.)
#ifndef PCB_SL_UNROLL
#define PCB_SL_UNROLL 4
#endif
#ifndef PCB_SL_NW4_MIN_A
#define PCB_SL_NW4_MIN_A 4096
#endif
constexpr int UNROLL = PCB_SL_UNROLL;

template <typename T, bool VEC, int NW>
__global__ __launch_bounds__(64 * NW) void k_sample_logits(DevParams p, SampleLogitsArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = xcd_contiguous_env((int)blockIdx.x, 0, p.B), tid = threadIdx.x, lane = tid & (WAVE - 1);
    const EvalGeom q{p.O, p.H, p.W, p.WW, p.B};
    const int H = p.H, W = p.W, WW = p.WW, HW = H * W, S = p.O * H * WW;
    const u64 *vm = (const u64 *)(p.state + (size_t)e * p.stateStride + p.offVm);
    const PolicyLds lds = carve_lds(smem, q);
    stage_bits(lds.vml, vm, q, tid, 64 * NW);
    if (tid == 0) *lds.bad = 0;
    __syncthreads();

    const T *row = (const T *)g.logits + (size_t)e * (size_t)(p.O * HW);
    const bool greedy = g.greedy != 0;
    if (pass1<T, VEC, NW, UNROLL, true>(row, lds, q, tid, greedy)) *lds.bad = 1;
    __syncthreads();
    if (tid >= WAVE) return;

    // ---- wavefront 0: the legal count, M, Z, the pick, the outputs
    int j0, j1;
    lane_run(S, lane, &j0, &j1);
    const auto [n, M, bits] = row_head(lds, q, j0, j1, lane);
    int a = 0;
    double logp = 0.0, ent = 0.0;
    if (n > 0 && bits) {
        // not a distribution: exactly the uniform draw of pcbenv_sample_actions
        int o, x, y;
        sample_action(vm, p, (int)g.first_env + e, lane, g.seed, g.step_index, &o, &x, &y);
        a = flatten_action(o, x, y, HW, W);
        logp = -log((double)n); ent = log((double)n);
    } else if (n > 0) {
        double mine = 0.0, tl = 0.0;
        combine_partials(lds, j0, j1, M, &mine, &tl);
        const double incl = wave_scan(mine, lane), Z = __shfl(incl, WAVE - 1);
        double excl = __shfl_up(incl, 1);
        if (lane == 0) excl = 0.0;
        const double tsum = wave_sum(tl), logZ = log(Z);
        ent = logZ - tsum / Z;
        if (greedy) {
            int cand = INT_MAX;
            for (int j = j0; j < j1; j++)
                if (lds.m[seg_slot(j)] == M) { cand = lds.first[seg_slot(j)]; break; }
            a = wave_min(cand);
            logp = -logZ;
        } else {
            const u64 rnd = draw_bits(g.seed, (int)g.first_env + e, g.step_index);
            const double uz = (double)(unsigned)(rnd >> 32) * 0x1p-32 * Z;
            // the lane whose run of segments holds u*Z (rounding can leave none: then the last lane with weight)
            const u64 owners = __ballot(mine > 0.0 && excl <= uz && uz < incl);
            const int ol = owners ? __ffsll((long long)owners) - 1 : 63 - __clzll((long long)__ballot(mine > 0.0));
            int J = -1;
            double rloc = 0.0;
            if (lane == ol) {
                double acc = excl;
                for (int j = j0; j < j1; j++) {
                    const int k = seg_slot(j);
                    const float s = lds.s[k];
                    if (s > 0.f) {
                        const float sc = seg_weight(lds.m[k], M);
                        const double sj = (double)s * (double)sc;
                        J = j; rloc = (uz - acc) / (double)sc;  // threshold in units of the segment's own weights
                        if (acc + sj > uz) break;
                        acc += sj;
                    }
                }
            }
            J = __shfl(J, ol); rloc = __shfl(rloc, ol);
            // re-read segment J: lane k holds column 64 w + k
            const Seg sg = segment(J, H, W, WW);
            const u64 word = seg_word(lds.vml, sg, H, WW);
            const bool legal = lane < sg.len && ((word >> lane) & 1ull);
            const float l = legal ? to_f32(row[sg.a0 + lane]) : -INFINITY;
            const float w = legal && l > -INFINITY ? seg_weight(l, lds.m[seg_slot(J)]) : 0.f;
            const float c = wave_scan(w, lane);
            const u64 hit = __ballot(w > 0.f && (double)c > rloc);
            // rounding can leave no element above the threshold: the segment's last legal element with weight
            const int k = hit ? __ffsll((long long)hit) - 1 : 63 - __clzll((long long)__ballot(w > 0.f));
            a = sg.a0 + k;
            logp = (double)__shfl(l, k) - (double)M - logZ;
        }
    }
    if (lane == 0) {
        int o, x, y;
        split_action(a, HW, W, &o, &x, &y);
        if (g.fmt == PCBENV_ACTION_FLAT) g.actions[e] = a;
        else { g.actions[3 * e] = o; g.actions[3 * e + 1] = x; g.actions[3 * e + 2] = y; }
        if (g.log_prob) g.log_prob[e] = (float)logp;
        if (g.entropy) g.entropy[e] = (float)ent;
        if (bits && g.errors) atomicOr(g.errors, bits);
    }
}

}  // namespace

int pcb_launch_sample_logits(const SampleLogitsLaunch &a) {
    const DevParams &d = a.d;
    const EvalGeom q{d.O, d.H, d.W, d.WW, d.B};
    select_launch(a.dtype, d.W, (uintptr_t)a.g.logits, d.O * d.H * d.W, PCB_SL_NW4_MIN_A, [&](auto t, auto vec, auto nw) {
        hipLaunchKernelGGL((k_sample_logits<typename decltype(t)::type, vec, nw>), dim3(d.B), dim3(64 * nw), lds_bytes(q), a.stream, d, a.g);
    });
    return 0;
}
