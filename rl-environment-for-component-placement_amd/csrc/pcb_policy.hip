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
// Weights are exp2((l - m) * log2 e) in float32, computed by one function in both passes, so the re-read of J sees
// exactly the weights its sum was made of.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "pcbenv.h"
#include "pcb_kernels.h"
#include "pcb_launch.h"
#include "pcb_policy_common.h"

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

// VEC: W % 4 == 0 and the logits 4-element aligned (every chunk of 4 is one vector load); otherwise one load per legal logit
template <typename T, bool VEC, int NW>
__global__ __launch_bounds__(64 * NW) void k_sample_logits(DevParams p, SampleLogitsArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = xcd_contiguous_env((int)blockIdx.x, 0, p.B), tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int H = p.H, W = p.W, WW = p.WW, HW = H * W, S = p.O * H * WW;
    const int nwords = (p.kind == PCBENV_SQUARE ? 1 : 2) * H * WW;
    const u64 *vm = (const u64 *)(p.state + (size_t)e * p.stateStride + p.offVm);
    u64 *vml = (u64 *)smem;  // the bit rows, [planes][H][WW]
    const int pad = seg_pad(S);
    float *sm_m = (float *)(vml + 2 * H * WW), *sm_s = sm_m + pad, *sm_t = sm_s + pad;
    int *sm_i = (int *)(sm_t + pad), *bad_flag = sm_i + pad;
    for (int i = tid; i < nwords; i += 64 * NW) vml[i] = vm[i];
    if (tid == 0) *bad_flag = 0;
    __syncthreads();

    const T *row = (const T *)g.logits + (size_t)e * (size_t)(p.O * HW);
    const int sub = lane & (SEG_LANES - 1), grp = tid >> 4;  // grp: this row's segment within a round
    constexpr int G = 64 * NW / SEG_LANES;                       // segments per round
    const bool greedy = g.greedy != 0;
    bool bad = false;
    for (int s0 = 0; s0 < S; s0 += G * UNROLL) {
        float v[UNROLL][4];
        unsigned nib[UNROLL];
        int a0[UNROLL];
        #pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const int j = s0 + u * G + grp;
            nib[u] = 0u; a0[u] = 0;
            if (j < S) {
                const Seg sg = segment(j, H, W, WW);
                const int rem = sg.len - 4 * sub;
                const unsigned word4 = (unsigned)(seg_word(vml, sg, H, WW) >> (4 * sub)) & 15u;
                nib[u] = rem <= 0 ? 0u : rem >= 4 ? word4 : word4 & ((1u << rem) - 1u);
                a0[u] = sg.a0 + 4 * sub;
            }
            if (VEC) {
                if (nib[u]) load4(row + a0[u], v[u]);
            } else {
                #pragma unroll
                for (int i = 0; i < 4; i++)
                    if ((nib[u] >> i) & 1u) v[u][i] = to_f32(row[a0[u] + i]);
            }
        }
        #pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            float lm = -INFINITY;
            #pragma unroll
            for (int i = 0; i < 4; i++)
                if ((nib[u] >> i) & 1u) { bad |= !(v[u][i] < INFINITY); lm = fmaxf(lm, v[u][i]); }
            const float m = row_max(lm);
            float sw = 0.f, st = 0.f;
            int first = INT_MAX;
            if (m > -INFINITY) {
                #pragma unroll
                for (int i = 3; i >= 0; i--) {
                    const float l = v[u][i];
                    if (((nib[u] >> i) & 1u) && l > -INFINITY) {
                        const float d = l - m, w = seg_weight(l, m);
                        sw += w; st += w * d;
                        if (l == m) first = a0[u] + i;
                    }
                }
            }
            sw = row_sum(sw); st = row_sum(st);
            if (greedy) first = row_min(first);
            const int j = s0 + u * G + grp;
            if (sub == 0 && j < S) { const int k = seg_slot(j); sm_m[k] = m; sm_s[k] = sw; sm_t[k] = st; sm_i[k] = first; }
        }
    }
    if (bad) *bad_flag = 1;
    __syncthreads();
    if (tid >= WAVE) return;

    // ---- wavefront 0: the legal count, M, Z, the pick, the outputs
    int cnt = 0;
    for (int i = lane; i < nwords; i += WAVE) cnt += __popcll(vml[i]);
    const int total = __builtin_amdgcn_readlane(wave_inclusive_scan(cnt, lane), WAVE - 1);
    const bool mirrored = p.kind == PCBENV_PIN || p.kind == PCBENV_SPATIAL;  // orientations 2, 3 reuse planes 0, 1
    const int n = mirrored ? 2 * total : total;
    const int per = (S + WAVE - 1) / WAVE, j0 = min(lane * per, S), j1 = min(j0 + per, S);
    float lm = -INFINITY;
    for (int j = j0; j < j1; j++) lm = fmaxf(lm, sm_m[seg_slot(j)]);
    const float M = wave_max(lm);
    const unsigned bits = n == 0 ? 0u : *bad_flag ? 1u : M == -INFINITY ? 2u : 0u;
    int a = 0;
    double logp = 0.0, ent = 0.0;
    if (n > 0 && bits) {
        // not a distribution: exactly the uniform draw of pcbenv_sample_actions
        int o, x, y;
        Team<64>::sample_action(vm, p, (int)g.first_env + e, lane, g.seed, g.step_index, &o, &x, &y);
        a = o * HW + x * W + y;
        logp = -log((double)n); ent = log((double)n);
    } else if (n > 0) {
        double mine = 0.0, tl = 0.0;
        for (int j = j0; j < j1; j++) {
            const int k = seg_slot(j);
            const float s = sm_s[k];
            if (s > 0.f) {
                const float m = sm_m[k], sc = seg_weight(m, M);
                mine += (double)s * (double)sc;
                tl += (double)sc * ((double)sm_t[k] + (double)s * ((double)m - (double)M));
            }
        }
        const double incl = wave_scan(mine, lane), Z = __shfl(incl, WAVE - 1);
        double excl = __shfl_up(incl, 1);
        if (lane == 0) excl = 0.0;
        const double tsum = wave_sum(tl), logZ = log(Z);
        ent = logZ - tsum / Z;
        if (greedy) {
            int cand = INT_MAX;
            for (int j = j0; j < j1; j++)
                if (sm_m[seg_slot(j)] == M) { cand = sm_i[seg_slot(j)]; break; }
            a = wave_min(cand);
            logp = -logZ;
        } else {
            const u64 rnd = Team<64>::mix64(Team<64>::mix64(g.seed ^ 0x9E3779B97F4A7C15ull * ((u64)((int)g.first_env + e) + 1)) + g.step_index);
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
                    const float s = sm_s[k];
                    if (s > 0.f) {
                        const float sc = seg_weight(sm_m[k], M);
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
            const u64 word = seg_word(vml, sg, H, WW);
            const bool legal = lane < sg.len && ((word >> lane) & 1ull);
            const float l = legal ? to_f32(row[sg.a0 + lane]) : -INFINITY;
            const float w = legal && l > -INFINITY ? seg_weight(l, sm_m[seg_slot(J)]) : 0.f;
            const float c = wave_scan(w, lane);
            const u64 hit = __ballot(w > 0.f && (double)c > rloc);
            // rounding can leave no element above the threshold: the segment's last legal element with weight
            const int k = hit ? __ffsll((long long)hit) - 1 : 63 - __clzll((long long)__ballot(w > 0.f));
            a = sg.a0 + k;
            logp = (double)__shfl(l, k) - (double)M - logZ;
        }
    }
    if (lane == 0) {
        const int o = a / HW, x = (a - o * HW) / W, y = a - o * HW - x * W;
        if (g.fmt == PCBENV_ACTION_FLAT) g.actions[e] = a;
        else { g.actions[3 * e] = o; g.actions[3 * e + 1] = x; g.actions[3 * e + 2] = y; }
        if (g.log_prob) g.log_prob[e] = (float)logp;
        if (g.entropy) g.entropy[e] = (float)ent;
        if (bits && g.errors) atomicOr(g.errors, bits);
    }
}

template <typename T, bool VEC>
void launch(const SampleLogitsLaunch &a, size_t lds) {
    const DevParams &d = a.d;
    if (d.O * d.H * d.W >= PCB_SL_NW4_MIN_A) hipLaunchKernelGGL((k_sample_logits<T, VEC, 4>), dim3(d.B), dim3(256), lds, a.stream, d, a.g);
    else hipLaunchKernelGGL((k_sample_logits<T, VEC, 1>), dim3(d.B), dim3(64), lds, a.stream, d, a.g);
}

}  // namespace

int pcb_launch_sample_logits(const SampleLogitsLaunch &a) {
    const DevParams &d = a.d;
    const size_t lds = lds_bytes(d.H, d.WW, d.O * d.H * d.WW);
    const bool f32 = a.dtype == PCBENV_LOGITS_F32;
    const bool vec = d.W % 4 == 0 && (uintptr_t)a.g.logits % (f32 ? 16 : 8) == 0;
    if (f32) { if (vec) launch<float, true>(a, lds); else launch<float, false>(a, lds); }
    else { if (vec) launch<bf16_bits, true>(a, lds); else launch<bf16_bits, false>(a, lds); }
    return 0;
}
