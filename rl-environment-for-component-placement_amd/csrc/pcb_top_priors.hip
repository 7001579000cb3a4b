// pcb_top_priors.hip -- k_top_priors and its entry point pcbenv_top_priors (include/pcbenv_priors.h): the K largest legal
// logits of every row in a defined order, with their probabilities under the row's masked categorical (what
// pcbenv/search.py:top_priors does with a stable sort over every logit).  Part of libpcbenv.so (CDNA4 / gfx950 only); a
// translation unit of its own, host side included, so that nothing here can change the builds of the other kernels or of
// the other entry points.
//
// One workgroup per row (xcd_contiguous_env), four wavefronts when A = O*H*W >= 4096, otherwise one.  The head is that of
// k_evaluate_logits, from pcb_policy_common.h unchanged: the bit rows staged into LDS, pass 1 (per segment max and sum),
// row_head (legal count n, row maximum M, the bad-row bits) and Z in float64.  What is decided about a candidate is
// pcb_topk.h, the text tools/topk_model_check.cpp composes on the CPU; here are the loads and the reductions around it.
//   select   four rounds of 8 bits over the keys (pcb_topk::key_of) of the legal logits: a round re-reads the row through
//            load_chunk and counts digits into a 256-bin histogram in LDS with integer atomics (order-independent, so
//            deterministic); wavefront 0 picks the bin that holds the rank.  The row is not staged -- at c5 it is 256 KiB
//            -- so the re-reads come from cache or memory.  Before the rounds the same select runs over the segments'
//            maxima (pass 1 left them in LDS): the k-th largest of those is a floor under the k-th candidate, and a segment
//            whose maximum lies below the floor, or from round 1 on below the prefix, is skipped without a load -- with
//            spread-out logits about k segments of the row are read again, with constant logits all of them.
//            The histogram is kept four times (copy = lane & 3), and a wavefront whose lanes all count the same digit --
//            constant logits, the worst case of a histogram -- adds its population once.
//   collect  one more pruned pass: keys above the threshold take a slot each (their order is fixed later), keys equal to it
//            are counted per segment.  Wavefront 0 scans those counts in segment (= flat index) order and lists the
//            segments that hold the first `need` equals; a wavefront per listed segment re-reads it, lane = column, and a
//            ballot gives every equal its place.  No place depends on how wavefronts were scheduled.
//   emit     wavefront 0: lane c ranks candidate c among the k <= 64 kept (pcb_topk::precedes), computes its prior in
//            float64 and writes row `rank`; lanes k .. K - 1 write the padding.  Every element of the outputs is written.
// A bad row (a legal NaN / +inf, or every legal logit -inf) and nothing else takes the uniform fallback: the first k legal
// actions in flat order, found from the bit rows alone with the scan and the ballots of `collect`.
#include <hip/hip_runtime.h>

#include "pcb_host.h"
#include "pcbenv_priors.h"
#include "pcb_launch.h"
#include "pcb_policy_common.h"
#include "pcb_topk.h"

static_assert(PCBENV_MAX_TREE_CHILDREN == pcb_topk::MAX_K && pcb_topk::MAX_K == WAVE, "one wavefront ranks the kept candidates");
static_assert(sizeof(pcbenv_top_priors_request) == 80 && offsetof(pcbenv_top_priors_request, stream) == 72, "pcbenv/_priors_lib.py:PcbenvTopPriorsRequest");

namespace {

using namespace pcb_topk;

// Segments per lane whose loads are issued before the first is used, and the smallest A launched with four wavefronts
// (as PCB_EV_UNROLL / PCB_EV_NW4_MIN_A).
#ifndef PCB_TP_UNROLL
#define PCB_TP_UNROLL 4
#endif
#ifndef PCB_TP_NW4_MIN_A
#define PCB_TP_NW4_MIN_A 4096
#endif
constexpr int UNROLL = PCB_TP_UNROLL;
constexpr int COPIES = 4;  // of the histogram

// what the kernel needs of a request; mask_bits null: the bit rows of row e are at state + e * stateStride + offVm
struct TopPriorsArgs {
    const void *logits;
    const u64 *mask_bits;
    const unsigned char *state;
    long long stateStride;
    int offVm, K;
    int *cand_count, *cand_actions;
    float *cand_prior;
    unsigned *errors;
};

// The LDS behind that of the forward kernels (lds_bytes(q), a multiple of 16): Z, the scalars one wavefront leaves for
// the others, the histogram, the kept candidates and the listed segments.
enum { SC_N, SC_BITS, SC_M, SC_PREFIX, SC_RANK, SC_ABOVE, SC_LISTED, SC_WORDS = 12 };
struct TopkLds { double *Z; int *sc; unsigned *hist, *ckey; int *cidx, *lseg, *lbase; };
__device__ inline TopkLds carve_topk(const PolicyLds &l) {
    TopkLds x;
    x.Z = (double *)(l.bad + 4);  // carve_lds ends with the 16 bytes of `bad`
    x.sc = (int *)(x.Z + 2);
    x.hist = (unsigned *)(x.sc + SC_WORDS);
    x.ckey = x.hist + COPIES * BINS;
    x.cidx = (int *)(x.ckey + MAX_K); x.lseg = x.cidx + MAX_K; x.lbase = x.lseg + MAX_K;
    return x;
}
inline size_t topk_lds_bytes(const EvalGeom &q) { return lds_bytes(q) + 16 + 4 * SC_WORDS + 4 * COPIES * BINS + 4 * 4 * MAX_K; }

__device__ inline int row_add(int v) {  // all-reduce over the 16 lanes of a DPP row
    v += dpp_i<0x128>(v); v += dpp_i<0x124>(v); v += dpp_i<0x122>(v); v += dpp_i<0x121>(v);
    return v;
}

// Every chunk of the row in the round structure of pass1: keep(largest key of segment j) says whether segment j is read;
// f(nib, v, a0, j) gets this lane's legal bits, values and first flat index of its chunk of segment j (nib 0: a segment
// not kept, or beyond the row).  Every lane of the workgroup makes the same calls of f.
template <typename T, bool VEC, int NW, class Keep, class F>
__device__ inline void for_chunks(const T *row, const PolicyLds &l, const EvalGeom &q, int tid, Keep keep, F f) {
    const int S = q.O * q.H * q.WW, sub = tid & (SEG_LANES - 1), grp = tid >> 4;
    constexpr int G = 64 * NW / SEG_LANES;
    for (int s0 = 0; s0 < S; s0 += G * UNROLL) {
        float v[UNROLL][4];
        unsigned nib[UNROLL];
        int a0[UNROLL], cols[UNROLL];
        #pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const int j = s0 + u * G + grp;
            const bool none = j >= S || !keep(key_of(l.m[seg_slot(min(j, S - 1))]));
            nib[u] = load_chunk<T, VEC>(row, l.vml, q, j, S, sub, none, v[u], &a0[u], &cols[u]);
        }
        #pragma unroll
        for (int u = 0; u < UNROLL; u++) f(nib[u], v[u], a0[u], s0 + u * G + grp);
    }
}

// One key per lane (valid: the lane has one) into the histogram; every lane of the wavefront calls.  A wavefront whose
// keys all have the same digit adds its population once.
__device__ inline void count_digit(unsigned *hist, bool valid, unsigned d, int lane) {
    const u64 act = __ballot(valid);
    if (act == 0ull) return;
    const int first = __ffsll((long long)act) - 1;
    const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)d, first);
    if (__ballot(valid && d == d0) == act) {
        if (lane == first) atomicAdd(&hist[COPIES * d0 + (lane & (COPIES - 1))], (unsigned)__popcll(act));
    } else if (valid) {
        atomicAdd(&hist[COPIES * d + (lane & (COPIES - 1))], 1u);
    }
}

template <typename T, bool VEC, int NW>
__global__ __launch_bounds__(64 * NW) void k_top_priors(EvalGeom q, TopPriorsArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NT = 64 * NW;
    const int e = xcd_contiguous_env((int)blockIdx.x, 0, q.rows), tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const int H = q.H, W = q.W, WW = q.WW, S = q.O * H * WW, K = g.K;
    const PolicyLds lds = carve_lds(smem, q);
    const TopkLds x = carve_topk(lds);
    const u64 *bits_src = g.mask_bits ? g.mask_bits + (size_t)e * (size_t)(2 * H * WW)
                                      : (const u64 *)(g.state + (size_t)e * (size_t)g.stateStride + g.offVm);
    stage_bits(lds.vml, bits_src, q, tid, NT);
    if (tid == 0) { *lds.bad = 0; x.sc[SC_ABOVE] = 0; x.sc[SC_LISTED] = 0; }
    __syncthreads();

    const T *row = (const T *)g.logits + (size_t)e * (size_t)(q.O * H * W);
    if (pass1<T, VEC, NW, UNROLL, false>(row, lds, q, tid, false)) *lds.bad = 1;
    __syncthreads();

    // ---- wavefront 0: the legal count, M, the bad-row bits and Z, left in LDS for the others
    int j0, j1;
    lane_run(S, lane, &j0, &j1);
    if (tid < WAVE) {
        const auto [n_, M_, bits_] = row_head(lds, q, j0, j1, lane);
        double mine = 0.0, tl = 0.0;
        if (n_ > 0 && !bits_) combine_partials(lds, j0, j1, M_, &mine, &tl);
        const double Zsum = wave_sum(mine);
        if (lane == 0) { x.sc[SC_N] = n_; x.sc[SC_BITS] = (int)bits_; x.sc[SC_M] = __float_as_int(M_); *x.Z = Zsum; }
    }
    __syncthreads();
    const int n = x.sc[SC_N], k = kept_count(K, n);
    const unsigned bad_bits = (unsigned)x.sc[SC_BITS];
    const bool uniform = bad_bits != 0u;
    const float M = __int_as_float(x.sc[SC_M]);

    // ---- the key of the k-th candidate, and how many candidates with exactly that key are kept
    unsigned threshold = 0u;
    int need = k;  // a bad row: the first k legal actions
    int *eq = (int *)lds.t;  // per segment slot, the legal logits equal to the threshold (pass 1's t has been combined)
    if (k > 0 && !uniform) {
        // A radix select: the rank-th largest of the keys `feed(prefix, r)` counts in round r (count_digit on those that
        // agree with the prefix) -> its key, and its rank among the keys equal to it.
        auto select = [&](unsigned rank, auto feed, unsigned *found) {
            unsigned prefix = 0u;
            for (int r = 0; r < ROUNDS; r++) {
                for (int i = tid; i < COPIES * BINS; i += NT) x.hist[i] = 0u;
                __syncthreads();
                feed(prefix, r);
                __syncthreads();
                if (tid < WAVE) {  // lane L: digits 255 - 4 L .. 252 - 4 L, the copies summed
                    unsigned h[4];
                    #pragma unroll
                    for (int t = 0; t < 4; t++) {
                        const uint4 c = *(const uint4 *)(x.hist + COPIES * digit_of_lane(lane, t));
                        h[t] = c.x + c.y + c.z + c.w;
                    }
                    const int mine = (int)(h[0] + h[1] + h[2] + h[3]), incl = group_inclusive_scan<WAVE>(mine, lane);
                    int t;
                    unsigned rest;
                    if ((unsigned)(incl - mine) < rank && choose_bin4(h, (unsigned)(incl - mine), rank, &t, &rest)) {  // one lane: the rank falls among its four
                        x.sc[SC_PREFIX] = (int)extend_prefix(prefix, digit_of_lane(lane, t), r);
                        x.sc[SC_RANK] = (int)rest;
                    }
                }
                __syncthreads();
                prefix = (unsigned)x.sc[SC_PREFIX]; rank = (unsigned)x.sc[SC_RANK];
            }
            *found = prefix;
            return rank;
        };
        // The floor: the k-th largest of the segments' maxima (they are in LDS: no load) is a legal logit with at least k
        // legal logits at or above it, so nothing below it can be kept, and a segment whose maximum is below it is never
        // read again.  With spread-out logits that leaves about k segments of the row.  Fewer than k segments: no floor.
        unsigned low = 0u;
        if (S >= k) {
            select((unsigned)k, [&](unsigned prefix, int r) {
                for (int j = tid; j - tid < S; j += NT) {
                    const unsigned key = key_of(lds.m[seg_slot(min(j, S - 1))]);
                    count_digit(x.hist, j < S && in_prefix(key, prefix, r), digit_of(key, r), lane);
                }
            }, &low);
        }
        const unsigned rank = select((unsigned)k, [&](unsigned prefix, int r) {
            for_chunks<T, VEC, NW>(row, lds, q, tid, [&](unsigned mk) { return may_hold_kept(mk, low) && may_hold_prefix(mk, prefix, r); },
                                   [&](unsigned nib, const float *v, int, int) {
                #pragma unroll
                for (int i = 0; i < 4; i++) {
                    const unsigned key = ((nib >> i) & 1u) ? key_of(v[i]) : 0u;
                    count_digit(x.hist, ((nib >> i) & 1u) && key >= low && in_prefix(key, prefix, r), digit_of(key, r), lane);
                }
            });
        }, &threshold);
        need = (int)rank;

        // ---- collect: keys above the threshold take a slot; equals are counted per segment
        for_chunks<T, VEC, NW>(row, lds, q, tid, [&](unsigned mk) { return may_hold_kept(mk, threshold); },
                               [&](unsigned nib, const float *v, int a0, int j) {
            int equals = 0;
            #pragma unroll
            for (int i = 0; i < 4; i++) {
                if ((nib >> i) & 1u) {
                    const unsigned key = key_of(v[i]);
                    if (key > threshold) {
                        const int slot = atomicAdd(&x.sc[SC_ABOVE], 1);
                        if (slot < MAX_K) { x.ckey[slot] = key; x.cidx[slot] = a0 + i; }
                    } else if (key == threshold) {
                        equals++;
                    }
                }
            }
            equals = row_add(equals);
            if ((tid & (SEG_LANES - 1)) == 0 && j < S) eq[seg_slot(j)] = equals;
        });
        __syncthreads();
    }
    const int above = k - need;  // kept candidates with a key above the threshold

    // ---- list the segments that hold the first `need` equals (a bad row: legal actions), in flat-index order
    if (k > 0 && tid < WAVE) {
        int total = 0;
        for (int j = j0; j < j1; j++) {
            const Seg sg = segment(j, H, W, WW);
            total += uniform ? __popcll(seg_word(lds.vml, sg, H, WW) & low_bits(sg.len)) : eq[seg_slot(j)];
        }
        int before = group_inclusive_scan<WAVE>(total, lane) - total;
        for (int j = j0; j < j1 && take_tie(before, need); j++) {
            const Seg sg = segment(j, H, W, WW);
            const int c = uniform ? __popcll(seg_word(lds.vml, sg, H, WW) & low_bits(sg.len)) : eq[seg_slot(j)];
            if (c > 0) {
                const int slot = atomicAdd(&x.sc[SC_LISTED], 1);
                if (slot < MAX_K) { x.lseg[slot] = j; x.lbase[slot] = before; }
                before += c;
            }
        }
    }
    __syncthreads();
    if (k > 0) {
        const int listed = min(x.sc[SC_LISTED], MAX_K);
        for (int t = wave; t < listed; t += NW) {  // lane = column of the listed segment
            const int j = x.lseg[t], before = x.lbase[t];
            const Seg sg = segment(j, H, W, WW);
            const bool legal = (seg_word(lds.vml, sg, H, WW) & low_bits(sg.len)) >> lane & 1ull;
            const unsigned key = legal && !uniform ? key_of(to_f32(row[sg.a0 + lane])) : 0u;
            const bool hit = legal && key == threshold;
            const int place = before + __popcll(__ballot(hit) & ((1ull << lane) - 1ull));
            if (hit && take_tie(place, need)) { x.ckey[above + place] = key; x.cidx[above + place] = sg.a0 + lane; }
        }
    }
    __syncthreads();
    if (tid >= WAVE) return;

    // ---- wavefront 0: rank the kept candidates, their priors, the outputs
    const unsigned key = lane < k ? x.ckey[lane] : 0u;
    const int idx = lane < k ? x.cidx[lane] : 0;
    int pos = lane;
    if (lane < k) {
        pos = 0;
        for (int c = 0; c < k; c++) pos += precedes(x.ckey[c], x.cidx[c], key, idx) ? 1 : 0;
    }
    if (lane < K) {
        int o = 0, xx = 0, y = 0;
        float p = 0.f;
        if (lane < k) {
            action_of(idx, H * W, W, &o, &xx, &y);
            p = uniform ? uniform_prior(n) : prior(value_of(key), M, *x.Z);
        }
        const size_t at = (size_t)e * (size_t)K + (size_t)pos;
        g.cand_actions[3 * at] = o; g.cand_actions[3 * at + 1] = xx; g.cand_actions[3 * at + 2] = y;
        g.cand_prior[at] = p;
    }
    if (lane == 0) {
        g.cand_count[e] = k;
        if (bad_bits && g.errors) atomicOr(g.errors, bad_bits);
    }
}

}  // namespace

// ---- pcbenv_top_priors -------------------------------------------------------------------------------------------
// As the policy entry points of pcbenv_api.hip: every argument check before a device is touched, in the order the header
// gives, the null handle behind what needs none; then one launch.
extern "C" int pcbenv_top_priors(const pcbenv *cenv, const pcbenv_top_priors_request *r) {
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    if (!r) return fail(env, PCBENV_EINVAL, "null request");
    if (r->struct_size != (uint32_t)sizeof(pcbenv_top_priors_request)) return fail(env, PCBENV_EINVAL, "struct_size is not sizeof(pcbenv_top_priors_request)");
    if (r->logits_dtype != PCBENV_LOGITS_F32 && r->logits_dtype != PCBENV_LOGITS_BF16) return fail(env, PCBENV_EINVAL, "unknown logits dtype");
    if (r->num_candidates < 1 || r->num_candidates > PCBENV_MAX_TREE_CHILDREN) return fail(env, PCBENV_EINVAL, "num_candidates must be in [1, 64]");
    if (r->reserved != 0) return fail(env, PCBENV_EINVAL, "reserved must be 0");
    if (r->num_rows < 0 || r->num_rows > INT32_MAX) return fail(env, PCBENV_EINVAL, "num_rows out of range");
    if (!r->logits || !r->cand_count || !r->cand_actions || !r->cand_prior) return fail(env, PCBENV_EINVAL, "null logits, cand_count, cand_actions or cand_prior");
    if ((uintptr_t)r->logits % (r->logits_dtype == PCBENV_LOGITS_F32 ? 4 : 2) != 0) return fail(env, PCBENV_EINVAL, "logits pointer not aligned to its element size");
    if ((uintptr_t)r->mask_bits % 8 != 0) return fail(env, PCBENV_EINVAL, "mask bits pointer not aligned to 8 bytes");
    if ((((uintptr_t)r->cand_count | (uintptr_t)r->cand_actions | (uintptr_t)r->cand_prior) & 3u) != 0)
        return fail(env, PCBENV_EINVAL, "cand_count, cand_actions and cand_prior must be 4-byte aligned");
    if (!env) return fail(0, PCBENV_EINVAL, "null handle");
    const DevParams &d = env->dp;
    const bool own_rows = r->mask_bits == 0;  // the legal sets of the handle's current state set
    if (own_rows && r->num_rows != d.B) return fail(env, PCBENV_EINVAL, "without mask_bits, num_rows must be num_envs");
    if (own_rows && !env->bound) return fail(env, PCBENV_ESTATE, "pcbenv_bind_buffers has not been called");
    if (r->num_rows == 0) return PCBENV_OK;
    DEVICE_GUARD(env);
    hipStream_t s = (hipStream_t)r->stream;
    // A captured launch would keep reading the state set that was current at capture time (as pcbenv_sample_logits).
    if (own_rows && stream_capturing(s)) return fail(env, PCBENV_ESTATE, "pcbenv_top_priors without mask_bits cannot be captured into a graph");
    const EvalGeom q{d.O, d.H, d.W, d.WW, (int)r->num_rows};
    TopPriorsArgs a;
    a.logits = r->logits; a.mask_bits = (const u64 *)r->mask_bits;
    a.state = d.state; a.stateStride = d.stateStride; a.offVm = d.offVm;  // d.state: the current state set, as k_sample_logits reads it
    a.K = r->num_candidates; a.cand_count = r->cand_count; a.cand_actions = r->cand_actions; a.cand_prior = r->cand_prior;
    a.errors = (unsigned *)r->errors_dev;
    select_launch(r->logits_dtype, q.W, (uintptr_t)r->logits, q.O * q.H * q.W, PCB_TP_NW4_MIN_A, [&](auto t, auto vec, auto nw) {
        hipLaunchKernelGGL((k_top_priors<typename decltype(t)::type, vec, nw>), dim3(q.rows), dim3(64 * nw), topk_lds_bytes(q), s, q, a);
    });
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}
