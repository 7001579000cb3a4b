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
// four wavefronts when A = O*H*W >= 4096, otherwise one.  Segments (the up to 64 logits one mask word governs) and the
// 16-lane DPP rows that reduce them are those of k_sample_logits (pcb_policy_common.h).
//   forward   per segment (m = max, s = sum exp(l - m), t = sum exp(l - m) (l - m)) -> LDS; wavefront 0 combines them
//             in float64 (M, Z, sum p (l - M)) and counts the legal bits; the stored action's logit is read directly and
//             its bit checked.  (M, log Z, entropy, row status) go to `stats` for the backward kernel.
//   backward  one pass: a chunk of 4 with no legal bit stores zeros without loading; otherwise
//             p = exp2((l - M - log Z) log2 e), g = g_lp (1[i = a] - p) - g_H p (log p + Hrow), whole vectors stored.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "pcbenv.h"
#include "pcb_kernels.h"
#include "pcb_launch.h"
#include "pcb_policy_common.h"

namespace {

// Segments per lane whose loads are issued before the first is used (as PCB_SL_UNROLL), and the smallest A launched with
// four wavefronts.  -DPCB_EV_NT_STORES: the gradient is written with non-temporal stores (A/B builds only;
// profiles/evaluate_logits_ab.txt).
#ifndef PCB_EV_UNROLL
#define PCB_EV_UNROLL 4
#endif
#ifndef PCB_EV_NW4_MIN_A
#define PCB_EV_NW4_MIN_A 4096
#endif
constexpr int UNROLL = PCB_EV_UNROLL;

// row status in stats[4 r + 3]
constexpr float ROW_OK = 0.f, ROW_ZERO = 1.f, ROW_NO_ONE_HOT = 2.f;

__device__ inline bf16_bits to_bf16(float v) {  // round to nearest even; v is finite
    const unsigned u = __float_as_uint(v);
    return (bf16_bits)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
template <typename V> __device__ inline void store_vec(V *p, V v) {
#ifdef PCB_EV_NT_STORES
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ inline void store4(float *p, const float v[4]) { store_vec((f32x4 *)p, f32x4{v[0], v[1], v[2], v[3]}); }
__device__ inline void store4(bf16_bits *p, const float v[4]) {
    store_vec((u32x2 *)p, u32x2{(unsigned)to_bf16(v[0]) | ((unsigned)to_bf16(v[1]) << 16), (unsigned)to_bf16(v[2]) | ((unsigned)to_bf16(v[3]) << 16)});
}
__device__ inline void store1(float *p, float v) { *p = v; }
__device__ inline void store1(bf16_bits *p, float v) { *p = to_bf16(v); }

// the bit rows of row e -> LDS ([planes][H][WW]; square: plane 0 only)
__device__ inline void load_mask(u64 *vml, const EvalGeom &q, const u64 *mask_bits, int e, int tid, int nthreads) {
    const u64 *vm = mask_bits + (size_t)e * (size_t)(2 * q.H * q.WW);
    const int nwords = (q.O == 1 ? 1 : 2) * q.H * q.WW;
    for (int i = tid; i < nwords; i += nthreads) vml[i] = vm[i];
}
// this lane's 4 columns of segment j: the first flat index, how many of them exist (0 beyond the segment's length or the
// last segment) and the legal bits of those
__device__ inline unsigned lane_nibble(const u64 *vml, const EvalGeom &q, int j, int S, int sub, int *a0, int *cols) {
    *a0 = 0; *cols = 0;
    if (j >= S) return 0u;
    const Seg sg = segment(j, q.H, q.W, q.WW);
    const unsigned word4 = (unsigned)(seg_word(vml, sg, q.H, q.WW) >> (4 * sub)) & 15u;
    *a0 = sg.a0 + 4 * sub;
    *cols = max(0, min(4, sg.len - 4 * sub));
    return word4 & ((1u << *cols) - 1u);
}
// flat action of row e, or -1 when it is out of range; *legal: its bit
__device__ inline int stored_action(const u64 *vml, const EvalGeom &q, const int *actions, int fmt, int e, bool *legal) {
    const int HW = q.H * q.W;
    int o, x, y;
    if (fmt == PCBENV_ACTION_FLAT) {
        const int a = actions[e];
        if (a < 0 || a >= q.O * HW) { *legal = false; return -1; }
        o = a / HW; x = (a - o * HW) / q.W; y = a - o * HW - x * q.W;
    } else {
        o = actions[3 * (size_t)e]; x = actions[3 * (size_t)e + 1]; y = actions[3 * (size_t)e + 2];
        if (o < 0 || o >= q.O || x < 0 || x >= q.H || y < 0 || y >= q.W) { *legal = false; return -1; }
    }
    *legal = (vml[(o & 1) * q.H * q.WW + x * q.WW + (y >> 6)] >> (y & 63)) & 1ull;
    return o * HW + x * q.W + y;
}

// VEC: W % 4 == 0 and the logits 4-element aligned (every chunk of 4 is one vector load); otherwise one load per legal logit
template <typename T, bool VEC, int NW>
__global__ __launch_bounds__(64 * NW) void k_evaluate_logits(EvalGeom q, EvalLogitsArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = xcd_contiguous_env((int)blockIdx.x, 0, q.rows), tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int H = q.H, W = q.W, WW = q.WW, S = q.O * H * WW;
    u64 *vml = (u64 *)smem;
    const int pad = seg_pad(S);
    float *sm_m = (float *)(vml + 2 * H * WW), *sm_s = sm_m + pad, *sm_t = sm_s + pad;
    int *bad_flag = (int *)(sm_t + pad);
    load_mask(vml, q, g.mask_bits, e, tid, 64 * NW);
    if (tid == 0) *bad_flag = 0;
    __syncthreads();

    const T *row = (const T *)g.logits + (size_t)e * (size_t)(q.O * H * W);
    // the stored action's logit, in flight under pass 1
    bool a_legal = false;
    int a = -1;
    float la = 0.f;
    if (tid == 0) {
        a = stored_action(vml, q, g.actions, g.fmt, e, &a_legal);
        if (a_legal) la = to_f32(row[a]);
    }
    const int sub = lane & (SEG_LANES - 1), grp = tid >> 4;
    constexpr int G = 64 * NW / SEG_LANES;  // segments per round
    bool bad = false;
    for (int s0 = 0; s0 < S; s0 += G * UNROLL) {
        float v[UNROLL][4];
        unsigned nib[UNROLL];
        #pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            int a0, cols;
            nib[u] = lane_nibble(vml, q, s0 + u * G + grp, S, sub, &a0, &cols);
            if (VEC) {
                if (nib[u]) load4(row + a0, v[u]);
            } else {
                #pragma unroll
                for (int i = 0; i < 4; i++)
                    if ((nib[u] >> i) & 1u) v[u][i] = to_f32(row[a0 + i]);
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
            if (m > -INFINITY) {
                #pragma unroll
                for (int i = 3; i >= 0; i--) {
                    const float l = v[u][i];
                    if (((nib[u] >> i) & 1u) && l > -INFINITY) {
                        const float d = l - m, w = seg_weight(l, m);
                        sw += w; st += w * d;
                    }
                }
            }
            sw = row_sum(sw); st = row_sum(st);
            const int j = s0 + u * G + grp;
            if (sub == 0 && j < S) { const int k = seg_slot(j); sm_m[k] = m; sm_s[k] = sw; sm_t[k] = st; }
        }
    }
    if (bad) *bad_flag = 1;
    __syncthreads();
    if (tid >= WAVE) return;

    // ---- wavefront 0: the legal count (columns beyond W never count), M, Z, the outputs
    const int per = (S + WAVE - 1) / WAVE, j0 = min(lane * per, S), j1 = min(j0 + per, S);
    int cnt = 0;
    float lm = -INFINITY;
    for (int j = j0; j < j1; j++) {
        const Seg sg = segment(j, H, W, WW);
        const u64 word = seg_word(vml, sg, H, WW);
        cnt += __popcll(sg.len == 64 ? word : word & ((1ull << sg.len) - 1ull));
        lm = fmaxf(lm, sm_m[seg_slot(j)]);
    }
    const int n = __builtin_amdgcn_readlane(wave_inclusive_scan(cnt, lane), WAVE - 1);
    const float M = wave_max(lm);
    const unsigned bad_bits = n == 0 ? 0u : *bad_flag ? 1u : M == -INFINITY ? 2u : 0u;
    double mine = 0.0, tl = 0.0;
    if (n > 0 && !bad_bits) {
        for (int j = j0; j < j1; j++) {
            const int k = seg_slot(j);
            const float s = sm_s[k];
            if (s > 0.f) {
                const float m = sm_m[k], sc = seg_weight(m, M);
                mine += (double)s * (double)sc;
                tl += (double)sc * ((double)sm_t[k] + (double)s * ((double)m - (double)M));
            }
        }
    }
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

// gradient of one legal logit.  c = M + log Z split as (M, log Z): lp = (l - M) - log Z keeps the cancellation in the
// first, exact-or-nearly-exact difference.  p = 0 (a legal -inf logit, or underflow): the entropy term is 0, never NaN.
__device__ inline float grad_one(float l, float M, float logZ, float Hrow, float glp, float gH, bool is_action) {
    const float lp = (l - M) - logZ, p = exp2f(lp * LOG2E);
    const float ge = p > 0.f ? gH * (p * (lp + Hrow)) : 0.f;
    return glp * ((is_action ? 1.f : 0.f) - p) - ge;
}

template <typename T, bool VEC, int NW>
__global__ __launch_bounds__(64 * NW) void k_evaluate_logits_backward(EvalGeom q, EvalLogitsBackwardArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = xcd_contiguous_env((int)blockIdx.x, 0, q.rows), tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int H = q.H, W = q.W, WW = q.WW, S = q.O * H * WW;
    u64 *vml = (u64 *)smem;
    load_mask(vml, q, g.mask_bits, e, tid, 64 * NW);
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
    const size_t base = (size_t)e * (size_t)(q.O * H * W);
    const T *row = (const T *)g.logits + base;
    T *out = (T *)g.grad_logits + base;
    const int sub = lane & (SEG_LANES - 1), grp = tid >> 4;
    constexpr int G = 64 * NW / SEG_LANES;
    for (int s0 = 0; s0 < S; s0 += G * UNROLL) {
        float v[UNROLL][4];
        unsigned nib[UNROLL];
        int a0[UNROLL], cols[UNROLL];  // cols: how many of this lane's 4 columns exist (all of them get a gradient)
        #pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            nib[u] = lane_nibble(vml, q, s0 + u * G + grp, S, sub, &a0[u], &cols[u]);
            if (zero_row) nib[u] = 0u;
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

size_t eval_lds_bytes(const EvalGeom &q) { return lds_bytes(q.H, q.WW, q.O * q.H * q.WW); }

template <typename T, bool VEC>
void launch_forward(const EvalLogitsLaunch &a) {
    const EvalGeom &q = a.q;
    if (q.O * q.H * q.W >= PCB_EV_NW4_MIN_A) hipLaunchKernelGGL((k_evaluate_logits<T, VEC, 4>), dim3(q.rows), dim3(256), eval_lds_bytes(q), a.stream, q, a.g);
    else hipLaunchKernelGGL((k_evaluate_logits<T, VEC, 1>), dim3(q.rows), dim3(64), eval_lds_bytes(q), a.stream, q, a.g);
}
template <typename T, bool VEC>
void launch_backward(const EvalLogitsBackwardLaunch &a) {
    const EvalGeom &q = a.q;
    const size_t lds = (size_t)16 * q.H * q.WW;
    if (q.O * q.H * q.W >= PCB_EV_NW4_MIN_A) hipLaunchKernelGGL((k_evaluate_logits_backward<T, VEC, 4>), dim3(q.rows), dim3(256), lds, a.stream, q, a.g);
    else hipLaunchKernelGGL((k_evaluate_logits_backward<T, VEC, 1>), dim3(q.rows), dim3(64), lds, a.stream, q, a.g);
}

}  // namespace

int pcb_launch_evaluate_logits(const EvalLogitsLaunch &a) {
    const bool f32 = a.dtype == PCBENV_LOGITS_F32;
    const bool vec = a.q.W % 4 == 0 && (uintptr_t)a.g.logits % (f32 ? 16 : 8) == 0;
    if (f32) { if (vec) launch_forward<float, true>(a); else launch_forward<float, false>(a); }
    else { if (vec) launch_forward<bf16_bits, true>(a); else launch_forward<bf16_bits, false>(a); }
    return 0;
}

int pcb_launch_evaluate_logits_backward(const EvalLogitsBackwardLaunch &a) {
    const bool f32 = a.dtype == PCBENV_LOGITS_F32;
    const uintptr_t both = (uintptr_t)a.g.logits | (uintptr_t)a.g.grad_logits;
    const bool vec = a.q.W % 4 == 0 && both % (f32 ? 16 : 8) == 0;
    if (f32) { if (vec) launch_backward<float, true>(a); else launch_backward<float, false>(a); }
    else { if (vec) launch_backward<bf16_bits, true>(a); else launch_backward<bf16_bits, false>(a); }
    return 0;
}
