// pcb_policy_common.h -- what the kernels that read a policy's logits through the legal-action bit rows share
// (k_sample_logits in pcb_policy.hip; k_evaluate_logits and its backward in pcb_policy_eval.hip): the segment
// addressing, the 16-byte / 8-byte chunk loads, the weight of a logit and the DPP row / wavefront reductions.
// Part of libpcbenv.so (CDNA4 / gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include "pcb_device.h"

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
__host__ __device__ inline size_t lds_bytes(int H, int WW, int S) { return (size_t)16 * H * WW + (size_t)16 * seg_pad(S) + 16; }

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
__device__ inline u64 seg_word(const u64 *vm, const Seg &g, int H, int WW) { return vm[(g.o & 1) * H * WW + g.x * WW + g.w]; }

}  // namespace
