// pcb_policy_common.h -- what the kernels that read a policy's logits through the legal-action bit rows share
// (k_sample_logits in pcb_policy.hip; k_evaluate_logits and its backward in pcb_policy_eval.hip; k_evaluate_visits and
// its backward in pcb_policy_visits.hip): the segment
// addressing, the bit-row staging, the chunk loads, the weight of a logit, pass 1 of the forward kernels, the pieces of
// their wavefront-0 combine, the DPP row / wavefront reductions and the launch selection.  The axis kernels
// (pcb_policy_axis.hip) take the weight, the wavefront reductions and the gradient of one logit from here.
// Part of libpcbenv.so (CDNA4 / gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <type_traits>

#include "pcbenv.h"
#include "pcb_device.h"
#include "pcb_launch.h"
#include "pcb_transition.h"

namespace {

constexpr float LOG2E = 1.44269504088896340736f;
constexpr int SEG_LANES = 16;  // lanes per segment in pass 1: one DPP row, 4 logits each

typedef unsigned short bf16_bits;
__device__ inline float to_f32(float v) { return v; }
__device__ inline float to_f32(bf16_bits v) { return __uint_as_float((unsigned)v << 16); }

// four consecutive logits from a 16-byte (float) / 8-byte (bf16) aligned address
__device__ inline void load4(const float *p, float v[4]) {
    const float4 q = *(const float4 *)p;
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
__device__ inline void load4(const bf16_bits *p, float v[4]) {
    const uint2 q = *(const uint2 *)p;
    v[0] = __uint_as_float(q.x << 16); v[1] = __uint_as_float(q.x & 0xFFFF0000u);
    v[2] = __uint_as_float(q.y << 16); v[3] = __uint_as_float(q.y & 0xFFFF0000u);
}

// weight of a legal logit relative to its segment's maximum (the one place it is computed)
__device__ inline float seg_weight(float l, float m) { return exp2f((l - m) * LOG2E); }

// what the backward kernels share: the gradient's bf16 rounding, its scalar store and the gradient of one logit
__device__ inline bf16_bits to_bf16(float v) {  // round to nearest even; v is finite
    const unsigned u = __float_as_uint(v);
    return (bf16_bits)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__device__ inline void store1(float *p, float v) { *p = v; }
__device__ inline void store1(bf16_bits *p, float v) { *p = to_bf16(v); }
// gradient of one legal logit.  c = M + log Z split as (M, log Z): lp = (l - M) - log Z keeps the cancellation in the
// first, exact-or-nearly-exact difference.  p = 0 (a legal -inf logit, or underflow): the entropy term is 0, never NaN.
__device__ inline float entropy_term(float l, float M, float logZ, float Hrow, float gH, float *p) {  // g_H p (log p + Hrow), and p
    const float lp = (l - M) - logZ;
    *p = exp2f(lp * LOG2E);
    return *p > 0.f ? gH * (*p * (lp + Hrow)) : 0.f;
}
__device__ inline float grad_one(float l, float M, float logZ, float Hrow, float glp, float gH, bool is_action) {
    float p;
    const float ge = entropy_term(l, M, logZ, Hrow, gH, &p);
    return glp * ((is_action ? 1.f : 0.f) - p) - ge;
}

// all-reduce over the 16 lanes of a DPP row (row_ror 8, 4, 2, 1); every lane must be active
template <int CTRL> __device__ inline float dpp_f(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false)); }
template <int CTRL> __device__ inline int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false); }
__device__ inline float row_max(float v) {
    v = fmaxf(v, dpp_f<0x128>(v)); v = fmaxf(v, dpp_f<0x124>(v)); v = fmaxf(v, dpp_f<0x122>(v)); v = fmaxf(v, dpp_f<0x121>(v));
    return v;
}
__device__ inline float row_sum(float v) {
    v += dpp_f<0x128>(v); v += dpp_f<0x124>(v); v += dpp_f<0x122>(v); v += dpp_f<0x121>(v);
    return v;
}
__device__ inline int row_min(int v) {
    v = min(v, dpp_i<0x128>(v)); v = min(v, dpp_i<0x124>(v)); v = min(v, dpp_i<0x122>(v)); v = min(v, dpp_i<0x121>(v));
    return v;
}
__device__ inline float wave_max(float v) { for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o)); return v; }
__device__ inline int wave_min(int v) { for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o)); return v; }
__device__ inline double wave_sum(double v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }
template <typename V> __device__ inline V wave_scan(V v, int lane) {  // inclusive, in lane order
    for (int d = 1; d < WAVE; d <<= 1) { const V t = __shfl_up(v, d); if (lane >= d) v += t; }
    return v;
}

__host__ __device__ inline int seg_slot(int j) { return j + (j >> 4); }  // one pad word per 16: wave 0 reads runs of 16
__host__ __device__ inline int seg_pad(int S) { return seg_slot(S) + 1; }

// segment j -> first flat index, valid columns and its mask word (bit y - 64 w of word = column y legal)
struct Seg { int a0, len, o, x, w; };
__device__ inline Seg segment(int j, int H, int W, int WW) {
    Seg g;
    g.w = WW == 1 ? 0 : (j & 1);
    const int ox = WW == 1 ? j : j >> 1;
    g.o = (ox >= H) + (ox >= 2 * H) + (ox >= 3 * H);  // O <= 4: no integer division
    g.x = ox - g.o * H;
    g.len = min(64, W - 64 * g.w);
    g.a0 = ox * W + 64 * g.w;
    return g;
}
__device__ inline u64 seg_word(const u64 *vml, const Seg &g, int H, int WW) { return vml[(g.o & 1) * H * WW + g.x * WW + g.w]; }

// the gradient's vector stores: four consecutive elements to a 16-byte (float) / 8-byte (bf16) aligned address
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

// A caller's action -- entry i of `actions`, [.., 3] (PCBENV_ACTION_TUPLE) or [..] (PCBENV_ACTION_FLAT) -- against the staged
// bit rows: its flat index, or -1 when it is out of range; *legal: its bit.  (The stored action of k_evaluate_logits, a
// target entry of k_evaluate_visits.)
__device__ inline int stored_action(const u64 *vml, const EvalGeom &q, const int *actions, int fmt, size_t i, bool *legal) {
    const int HW = q.H * q.W;
    int o, x, y;
    if (fmt == PCBENV_ACTION_FLAT) {
        const int a = actions[i];
        if (a < 0 || a >= q.O * HW) { *legal = false; return -1; }
        split_action(a, HW, q.W, &o, &x, &y);
    } else {
        o = actions[3 * i]; x = actions[3 * i + 1]; y = actions[3 * i + 2];
        if (o < 0 || o >= q.O || x < 0 || x >= q.H || y < 0 || y >= q.W) { *legal = false; return -1; }  // !PCB_ACTION_IN_RANGE, as it stood
    }
    *legal = PCB_LEGAL_BIT(vml, (o & 1) * q.H * q.WW, q.WW, x, y);
    return PCB_FLATTEN_ACTION(o, x, y, HW, q.W);
}

// The LDS of the forward kernels, carved the same way by both: the bit rows [2][H][WW], then per segment slot m, s, t and
// the first index of the max (the sampler's only), then the flag of a NaN / +inf legal logit.  The backward uses the
// bit rows alone.
struct PolicyLds { u64 *vml; float *m, *s, *t; int *first, *bad; };
__device__ inline PolicyLds carve_lds(unsigned char *smem, const EvalGeom &q) {
    const int pad = seg_pad(q.O * q.H * q.WW);
    PolicyLds l;
    l.vml = (u64 *)smem;
    l.m = (float *)(l.vml + 2 * q.H * q.WW); l.s = l.m + pad; l.t = l.s + pad;
    l.first = (int *)(l.t + pad); l.bad = l.first + pad;
    return l;
}
inline size_t lds_bytes(const EvalGeom &q) { return (size_t)16 * q.H * q.WW + (size_t)16 * seg_pad(q.O * q.H * q.WW) + 16; }

// one row's bit rows ([planes][H][WW] at src) -> LDS; O == 1: plane 0 only
__device__ inline void stage_bits(u64 *vml, const u64 *src, const EvalGeom &q, int tid, int nthreads) {
    const int nwords = (q.O == 1 ? 1 : 2) * q.H * q.WW;
    for (int i = tid; i < nwords; i += nthreads) vml[i] = src[i];
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

// this lane's chunk of segment j (its columns 4 sub .. 4 sub + 3) -> v; returns the legal bits, a0 / cols as lane_nibble
// (none: no legal bit, a0 and cols kept).  VEC: W % 4 == 0 and the logits 4-element aligned, one vector load per chunk
// with a legal bit; otherwise one load per legal logit.  Called UNROLL times before the first chunk is used.
template <typename T, bool VEC>
__device__ inline unsigned load_chunk(const T *row, const u64 *vml, const EvalGeom &q, int j, int S, int sub, bool none,
                                      float v[4], int *a0, int *cols) {
    unsigned nib = lane_nibble(vml, q, j, S, sub, a0, cols);
    if (none) nib = 0u;
    if (VEC) {
        if (nib) load4(row + *a0, v);
    } else {
        #pragma unroll
        for (int i = 0; i < 4; i++)
            if ((nib >> i) & 1u) v[i] = to_f32(row[*a0 + i]);
    }
    return nib;
}

// Pass 1 of the forward kernels: a 16-lane DPP row per segment, UNROLL segments' loads in flight per lane; per segment
// (m = max, s = sum exp(l - m), t = sum exp(l - m) (l - m) and, FIRST and greedy, the first index of the max) -> LDS.
// Returns whether one of this lane's legal logits was NaN or +inf.
template <typename T, bool VEC, int NW, int UNROLL, bool FIRST>
__device__ inline bool pass1(const T *row, const PolicyLds &l, const EvalGeom &q, int tid, bool greedy) {
    const int S = q.O * q.H * q.WW, sub = tid & (SEG_LANES - 1), grp = tid >> 4;  // grp: this row's segment within a round
    constexpr int G = 64 * NW / SEG_LANES;                                      // segments per round
    bool bad = false;
    for (int s0 = 0; s0 < S; s0 += G * UNROLL) {
        float v[UNROLL][4];
        unsigned nib[UNROLL];
        int a0[UNROLL], cols[UNROLL];
        #pragma unroll
        for (int u = 0; u < UNROLL; u++) nib[u] = load_chunk<T, VEC>(row, l.vml, q, s0 + u * G + grp, S, sub, false, v[u], &a0[u], &cols[u]);
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
                    const float lv = v[u][i];
                    if (((nib[u] >> i) & 1u) && lv > -INFINITY) {
                        const float d = lv - m, w = seg_weight(lv, m);
                        sw += w; st += w > 0.f ? w * d : 0.f;  // a zero weight contributes 0: l - m may be -inf, and 0 * -inf is NaN
                        if (FIRST && lv == m) first = a0[u] + i;
                    }
                }
            }
            sw = row_sum(sw); st = row_sum(st);
            if (FIRST && greedy) first = row_min(first);
            const int j = s0 + u * G + grp;
            if (sub == 0 && j < S) {
                const int k = seg_slot(j);
                l.m[k] = m; l.s[k] = sw; l.t[k] = st;
                if (FIRST) l.first[k] = first;
            }
        }
    }
    return bad;
}

// ---- wavefront 0 of the forward kernels; lane holds the run of segments [j0, j1)
__device__ inline void lane_run(int S, int lane, int *j0, int *j1) {
    const int per = (S + WAVE - 1) / WAVE;
    *j0 = min(lane * per, S); *j1 = min(*j0 + per, S);
}
// n: the legal count over all S segments (columns beyond W never count; orientations 2, 3 count their planes again),
// M: the largest legal logit, bits: the error bits (0 when n == 0; 1 a NaN / +inf legal logit; 2 every legal logit -inf).
// Segment j's mask word is vml[j mod 2 H WW] and its valid columns those of column word j & (WW - 1) (segment() and
// seg_word() without their arithmetic: this loop is serial work of wavefront 0).
struct RowHead { int n; float M; unsigned bits; };
__device__ inline u64 low_bits(int len) { return len >= 64 ? ~0ull : (1ull << len) - 1ull; }
__device__ inline RowHead row_head(const PolicyLds &l, const EvalGeom &q, int j0, int j1, int lane) {
    const int nw = 2 * q.H * q.WW;
    const u64 valid0 = low_bits(q.W), valid1 = low_bits(q.W - 64);
    int cnt = 0;
    float lm = -INFINITY;
    for (int j = j0, i = j0 % nw; j < j1; j++, i = i + 1 == nw ? 0 : i + 1) {
        cnt += __popcll(l.vml[i] & (j & (q.WW - 1) ? valid1 : valid0));
        lm = fmaxf(lm, l.m[seg_slot(j)]);
    }
    RowHead h;
    h.n = __builtin_amdgcn_readlane(group_inclusive_scan<WAVE>(cnt, lane), WAVE - 1);
    h.M = wave_max(lm);
    h.bits = h.n == 0 ? 0u : *l.bad ? 1u : h.M == -INFINITY ? 2u : 0u;
    return h;
}
// the lane's float64 partials of Z = sum s exp(m - M) (mine) and of sum exp(l - M) (l - M) (tl); each kernel reduces
// them its own way
__device__ inline void combine_partials(const PolicyLds &l, int j0, int j1, float M, double *mine, double *tl) {
    for (int j = j0; j < j1; j++) {
        const int k = seg_slot(j);
        const float s = l.s[k];
        if (s > 0.f) {
            const float m = l.m[k], sc = seg_weight(m, M);
            *mine += (double)s * (double)sc;
            *tl += (double)sc * ((double)l.t[k] + (double)s * ((double)m - (double)M));
        }
    }
}

// ---- launch selection: dtype -> T; W % 4 == 0 and `ptrs` (the logits pointer, or all the pointers ORed) aligned to 4
// elements -> VEC; A >= nw4_min_a -> four wavefronts (NW), otherwise one.  f(type_tag<T>, VEC, NW), the last two as
// std::integral_constant.
template <typename T> struct type_tag { typedef T type; };
template <typename F>
void select_launch(int dtype, int W, uintptr_t ptrs, int A, int nw4_min_a, F &&f) {
    const bool f32 = dtype == PCBENV_LOGITS_F32;
    const bool vec = W % 4 == 0 && ptrs % (f32 ? 16 : 8) == 0, nw4 = A >= nw4_min_a;
    auto with_nw = [&](auto t, auto v) {
        if (nw4) f(t, v, std::integral_constant<int, 4>());
        else f(t, v, std::integral_constant<int, 1>());
    };
    auto with_vec = [&](auto t) {
        if (vec) with_nw(t, std::true_type());
        else with_nw(t, std::false_type());
    };
    if (f32) with_vec(type_tag<float>());
    else with_vec(type_tag<bf16_bits>());
}

}  // namespace
