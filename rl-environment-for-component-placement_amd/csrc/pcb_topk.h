// pcb_topk.h -- the selection of pcbenv_top_priors, stated once: the order of two legal logits, the radix select that finds
// the K-th of them, the tie rule, the final rank and the prior of a kept action.  Plain C++17 that compiles alone, on the
// host and on the device: k_top_priors (pcb_top_priors.hip) composes the pieces below around its loads, its histogram in
// LDS and its wavefront scans, and tools/topk_model_check.cpp -- a CPU program under AddressSanitizer and UBSan --
// composes them serially over the rows of tests/top_priors_cases.py.  Everything here is integer work except prior().
//
// The order (include/pcbenv_priors.h): legal logits by value descending, compared as IEEE float32 values (-0.0 equals
// +0.0), ties to the lower flat index.  key_of maps a value to 32 bits whose unsigned order is that order, so the K-th
// largest is found by four rounds over 8 bits each, most significant first: a round counts, per digit, the keys that
// agree with the prefix chosen so far, and choose_bin4 walks the counts from the highest digit down to the one that
// holds the rank.  After round 3 the prefix is the key of the K-th candidate and the rank left over is how many
// candidates carry exactly that key: those with the lowest flat indices, take_tie.  The same select over the largest key
// of every segment (up to 64 consecutive logits) gives a floor first: the K-th largest of those has K legal logits at or
// above it, so keys below it are not counted and segments below it not read (may_hold_kept).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCB_TOPK_HD __host__ __device__
#else
#define PCB_TOPK_HD
#endif

namespace pcb_topk {

constexpr int MAX_K = 64;             // PCBENV_MAX_TREE_CHILDREN: one wavefront ranks the kept candidates
constexpr int ROUNDS = 4, BINS = 256;  // 8 bits per round
constexpr unsigned ERR_BAD = 1u;       // bit 0: a legal logit was NaN or +inf
constexpr unsigned ERR_ALL_NEG_INF = 2u;  // bit 1: every legal logit was -inf

PCB_TOPK_HD inline uint32_t bits_of(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
PCB_TOPK_HD inline float float_of(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }

// value -> key, unsigned order = value order; -0.0 is +0.0 first.  (No NaN comes here: a row with a legal NaN is a bad
// row and is not ordered by value.)  -inf gets the smallest key a legal logit can have.
PCB_TOPK_HD inline uint32_t key_of(float v) {
    uint32_t u = bits_of(v);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// key -> the value it came from (-0.0 comes back as +0.0)
PCB_TOPK_HD inline float value_of(uint32_t key) { return float_of((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key); }

// round r = 0 .. 3 looks at bits [shift, shift + 8) of the keys that agree with `prefix` in the bits above
PCB_TOPK_HD inline int round_shift(int r) { return 24 - 8 * r; }
PCB_TOPK_HD inline uint32_t bits_above(int r) { return r == 0 ? 0u : 0xFFFFFFFFu << (32 - 8 * r); }
PCB_TOPK_HD inline bool in_prefix(uint32_t key, uint32_t prefix, int r) { return (key & bits_above(r)) == prefix; }
PCB_TOPK_HD inline unsigned digit_of(uint32_t key, int r) { return (key >> round_shift(r)) & 255u; }
PCB_TOPK_HD inline uint32_t extend_prefix(uint32_t prefix, unsigned digit, int r) { return prefix | ((uint32_t)digit << round_shift(r)); }
// a segment whose largest key is max_key can hold a key in the prefix of round r, or one >= the floor / the threshold:
// otherwise it is not read again
PCB_TOPK_HD inline bool may_hold_prefix(uint32_t max_key, uint32_t prefix, int r) { return (max_key & bits_above(r)) >= prefix; }
PCB_TOPK_HD inline bool may_hold_kept(uint32_t max_key, uint32_t threshold) { return max_key >= threshold; }

// Four counts of consecutive digits, highest digit first, with `above` = how many keys of the prefix have a higher digit
// than h[0]'s: if the rank-th largest (rank >= 1) falls among them, *t = which of the four and *rest = its rank inside
// that digit.  The kernel gives every lane four digits and finds `above` by a scan; the model walks the 64 groups.
PCB_TOPK_HD inline bool choose_bin4(const unsigned h[4], unsigned above, unsigned rank, int *t, unsigned *rest) {
    for (int i = 0; i < 4; i++) {
        if (above + h[i] >= rank) { *t = i; *rest = rank - above; return true; }
        above += h[i];
    }
    return false;
}
PCB_TOPK_HD inline unsigned digit_of_lane(int group, int t) { return (unsigned)(BINS - 1 - 4 * group - t); }  // group 0 holds digits 255 .. 252

// Of the candidates whose key equals the threshold, `need` are kept: the one with `before` equals in front of it (in
// flat-index order) is kept if before < need, and comes at place (kept above the threshold) + before.
PCB_TOPK_HD inline bool take_tie(int before, int need) { return before < need; }

// candidate a = (key, flat index) comes before candidate b in the output
PCB_TOPK_HD inline bool precedes(uint32_t key_a, int idx_a, uint32_t key_b, int idx_b) {
    return key_a > key_b || (key_a == key_b && idx_a < idx_b);
}

PCB_TOPK_HD inline int kept_count(int K, int n) { return n < K ? n : K; }

// flat index a = o*H*W + x*W + y -> (o, x, y)
PCB_TOPK_HD inline void action_of(int a, int HW, int W, int *o, int *x, int *y) {
    *o = a / HW;
    const int r = a - *o * HW;
    *x = r / W; *y = r - *x * W;
}

// float32(exp(v - M) / Z) in float64, rounded once; M the largest legal logit (finite), Z the sum over the legal set
PCB_TOPK_HD inline float prior(float v, float M, double Z) { return (float)(exp((double)v - (double)M) / Z); }
// a bad row: the first k legal actions, each with float32(1.0 / n)
PCB_TOPK_HD inline float uniform_prior(int n) { return (float)(1.0 / (double)n); }

}  // namespace pcb_topk
