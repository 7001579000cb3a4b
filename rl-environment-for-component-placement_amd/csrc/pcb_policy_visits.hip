// pcb_policy_visits.hip -- k_evaluate_visits and k_evaluate_visits_backward with their entry points pcbenv_evaluate_visits
// and pcbenv_evaluate_visits_backward (include/pcbenv_train.h): the cross entropy of a policy's masked categorical against
// the visit counts of a searched move (the AlphaZero policy loss), its entropy, and their gradient with respect to the
// logits.  Part of libpcbenv.so (CDNA4 / gfx950 only); a translation unit of its own, host side included, so that nothing
// here can change the builds of the other kernels or of the other entry points.
//
// The distribution is that of k_evaluate_logits and so is the launch: one workgroup per row (xcd_contiguous_env), four
// wavefronts when A = O*H*W >= 4096, otherwise one; the bit rows staged into LDS, pass 1, row_head, combine_partials,
// load_chunk and the entropy term of the gradient are pcb_policy_common.h's, unchanged.  What differs is the target: up to
// 64 (visits, action) entries per row in place of one stored action.  What is decided about an entry is
// pcb_visit_targets.h, the text tools/visit_targets_check.cpp composes on the CPU.
//   forward   lane c < C of wavefront 0 takes entry c: it is tested against the staged bit rows and its logit loaded, in
//             flight under pass 1.  After the combine wavefront 0 sums T (int64) and sum visits_c (l_c - M) (float64) over
//             its lanes; cross_entropy = log Z - that sum / T.  (M, log Z, entropy, row status) go to `stats`.
//   backward  one pass, every element stored once with the vector stores of k_evaluate_logits_backward.  The <= 64
//             targets reach their elements through a target bit map in LDS, [O*H*WW] words laid out like the segments, and
//             a byte per word that counts the target bits before it (pcb_visit_targets.h: map_place, slot_of).  Wavefront
//             0 ORs every valid entry's bit in with an LDS atomic, scans the words' popcounts, and adds every entry's visits
//             into the slot of its bit (a 64-bit LDS atomic: duplicates add up exactly).  A chunk takes its target nibble as
//             it takes its legal nibble, and only an element whose target bit is set reads its slot and divides by T, once.
//             No search, no second store.  LDS: 16 H WW (bit rows) + 9 O H WW (target map, counts) + 528 bytes, 13.5 KB
//             at 128x128 with four orientations.
#include <hip/hip_runtime.h>

#include "pcb_host.h"
#include "pcbenv_train.h"
#include "pcb_launch.h"
#include "pcb_policy_common.h"
#include "pcb_visit_targets.h"

static_assert(PCBENV_MAX_TREE_CHILDREN == pcb_visits::MAX_TARGETS && pcb_visits::MAX_TARGETS == WAVE, "one wavefront holds a row's entries");
static_assert(sizeof(pcbenv_visits_request) == 128 && offsetof(pcbenv_visits_request, stream) == 120, "pcbenv/_train_lib.py:PcbenvVisitsRequest");

namespace {

using pcb_visits::Entry;

// Segments per lane whose loads are issued before the first is used, and the smallest A launched with four wavefronts
// (as PCB_EV_UNROLL / PCB_EV_NW4_MIN_A).
#ifndef PCB_VT_UNROLL
#define PCB_VT_UNROLL 4
#endif
#ifndef PCB_VT_NW4_MIN_A
#define PCB_VT_NW4_MIN_A 4096
#endif
constexpr int UNROLL = PCB_VT_UNROLL;

// row status in stats[4 r + 3]
constexpr float ROW_OK = 0.f, ROW_ZERO = 1.f, ROW_NO_TARGET = 2.f;

// what the kernels need of a request
struct VisitsArgs {
    const void *logits;
    const u64 *mask_bits;
    const int *visits, *actions;
    float *cross_entropy, *entropy, *stats;
    unsigned *errors;
    const float *grad_ce, *grad_entropy;
    void *grad_logits;
    int fmt, C;
};

__device__ inline long long wave_sum(long long v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }

// entry `lane` of row e against the staged bit rows (lane < C); *bad: it raises bit 2
__device__ inline Entry target_entry(const u64 *vml, const EvalGeom &q, const VisitsArgs &g, int e, int lane, bool *bad) {
    const size_t at = (size_t)e * (size_t)g.C + (size_t)lane;
    return pcb_visits::entry_of(g.visits[at], lane, [&](int) {
        bool legal;
        const int a = stored_action(vml, q, g.actions, g.fmt, at, &legal);
        return legal ? a : -1;
    }, bad);
}

template <typename T, bool VEC, int NW>
__global__ __launch_bounds__(64 * NW) void k_evaluate_visits(EvalGeom q, VisitsArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = xcd_contiguous_env((int)blockIdx.x, 0, q.rows), tid = threadIdx.x, lane = tid & (WAVE - 1);
    const PolicyLds lds = carve_lds(smem, q);
    stage_bits(lds.vml, g.mask_bits + (size_t)e * (size_t)(2 * q.H * q.WW), q, tid, 64 * NW);
    if (tid == 0) *lds.bad = 0;
    __syncthreads();

    const T *row = (const T *)g.logits + (size_t)e * (size_t)(q.O * q.H * q.W);
    // this lane's target entry; its logit is in flight under pass 1
    Entry te{-1, 0};
    bool t_bad = false;
    float lt = 0.f;
    if (tid < g.C) {
        te = target_entry(lds.vml, q, g, e, tid, &t_bad);
        if (te.index >= 0) lt = to_f32(row[te.index]);
    }
    if (pass1<T, VEC, NW, UNROLL, false>(row, lds, q, tid, false)) *lds.bad = 1;
    __syncthreads();
    if (tid >= WAVE) return;

    // ---- wavefront 0: the legal count, M, Z, the targets, the outputs
    int j0, j1;
    lane_run(q.O * q.H * q.WW, lane, &j0, &j1);
    const auto [n, M, bad_bits] = row_head(lds, q, j0, j1, lane);
    const bool ok = n > 0 && !bad_bits;  // the row is a distribution
    double mine = 0.0, tl = 0.0;
    if (ok) combine_partials(lds, j0, j1, M, &mine, &tl);
    const double Z = wave_sum(mine), tsum = wave_sum(tl);
    const long long total = wave_sum((long long)(ok ? te.visits : 0));
    const double wl = wave_sum(ok && te.index >= 0 ? pcb_visits::weighted_logit(te.visits, lt, M) : 0.0);
    const bool target_bad = __ballot(ok && t_bad) != 0ull;
    if (lane != 0) return;
    unsigned bits = bad_bits;
    float status = ROW_ZERO, statM = 0.f, statLogZ = 0.f;
    double ce = 0.0, ent = 0.0;
    if (n > 0 && bad_bits) {
        ce = ent = log((double)n);
    } else if (n > 0) {
        const double logZ = log(Z);
        ent = logZ - tsum / Z;
        statM = M; statLogZ = (float)logZ;
        if (target_bad) bits |= pcb_visits::ERR_TARGET;
        if (total > 0) { ce = logZ - wl / (double)total; status = ROW_OK; }
        else status = ROW_NO_TARGET;
    }
    if (g.cross_entropy) g.cross_entropy[e] = (float)ce;
    if (g.entropy) g.entropy[e] = (float)ent;
    if (g.stats) {
        float4 st;
        st.x = statM; st.y = statLogZ; st.z = (float)ent; st.w = status;
        *(float4 *)(g.stats + 4 * (size_t)e) = st;
    }
    if (bits && g.errors) atomicOr(g.errors, bits);
}

// the LDS of the backward kernel: the bit rows [2][H][WW], the target map [O*H*WW] (word j = segment j), T (16 bytes), the
// visits per slot [WAVE], the targets before each word [O*H*WW] bytes
inline size_t backward_lds_bytes(const EvalGeom &q) {
    const size_t S = (size_t)q.O * q.H * q.WW;
    return (size_t)16 * q.H * q.WW + 8 * S + 16 + (size_t)8 * WAVE + ((S + 15) & ~(size_t)15);
}

template <typename T, bool VEC, int NW>
__global__ __launch_bounds__(64 * NW) void k_evaluate_visits_backward(EvalGeom q, VisitsArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = xcd_contiguous_env((int)blockIdx.x, 0, q.rows), tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int S = q.O * q.H * q.WW;
    u64 *vml = (u64 *)smem, *tmap = vml + 2 * q.H * q.WW;
    long long *ttotal = (long long *)(tmap + S);
    unsigned long long *tsum = (unsigned long long *)(ttotal + 2);
    unsigned char *tbefore = (unsigned char *)(tsum + WAVE);
    stage_bits(vml, g.mask_bits + (size_t)e * (size_t)(2 * q.H * q.WW), q, tid, 64 * NW);
    for (int i = tid; i < S; i += 64 * NW) tmap[i] = 0ull;
    if (tid < WAVE) tsum[tid] = 0ull;
    const float4 st = *(const float4 *)(g.stats + 4 * (size_t)e);
    const float M = st.x, logZ = st.y, Hrow = st.z;
    const bool zero_row = st.w == ROW_ZERO;
    // ROW_NO_TARGET: the g_ce term is dropped
    const float gce = g.grad_ce && st.w == ROW_OK ? g.grad_ce[e] : 0.f, gH = g.grad_entropy ? g.grad_entropy[e] : 0.f;
    __syncthreads();
    // wavefront 0, entry `lane`: its bit into the map, the targets before each word, its visits into the slot of its bit
    // (the forward call found T > 0 where the row is ROW_OK; otherwise the map stays empty)
    Entry te{-1, 0};
    int tword = 0, tbit = 0;
    if (tid < WAVE) {
        bool bad = false;
        if (st.w == ROW_OK && lane < g.C) te = target_entry(vml, q, g, e, lane, &bad);
        const long long total = wave_sum((long long)te.visits);
        if (lane == 0) *ttotal = total;
        if (te.index >= 0) {
            pcb_visits::map_place(te.index, q.W, q.WW, &tword, &tbit);
            atomicOr((unsigned long long *)&tmap[tword], 1ull << tbit);
        }
    }
    __syncthreads();
    if (tid < WAVE) {
        int j0, j1, count = 0;
        lane_run(S, lane, &j0, &j1);
        for (int j = j0; j < j1; j++) count += __popcll(tmap[j]);
        int before = group_inclusive_scan<WAVE>(count, lane) - count;
        for (int j = j0; j < j1; j++) { tbefore[j] = (unsigned char)before; before += __popcll(tmap[j]); }
    }
    __syncthreads();
    if (te.index >= 0) atomicAdd(&tsum[pcb_visits::slot_of(tbefore[tword], tmap[tword], tbit)], (unsigned long long)te.visits);
    __syncthreads();
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
            const int j = s0 + u * G + grp;
            const unsigned hit = nib[u] ? (unsigned)(tmap[j] >> (4 * sub)) & nib[u] : 0u;  // nib != 0: j < S
            float gr[4];
            #pragma unroll
            for (int i = 0; i < 4; i++) {
                gr[i] = 0.f;
                if ((nib[u] >> i) & 1u) {
                    float p;
                    const float ge = entropy_term(v[u][i], M, logZ, Hrow, gH, &p);
                    const float pi = (hit >> i) & 1u ? pcb_visits::pi_of((long long)tsum[pcb_visits::slot_of(tbefore[j], tmap[j], 4 * sub + i)], *ttotal) : 0.f;
                    gr[i] = gce * (p - pi) - ge;
                }
            }
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

// Every argument check of the two calls, before a device is touched, in the order the header gives, the null handle last.
int visits_checks(pcbenv *env, const pcbenv_visits_request *r, bool backward) {
    if (!r) return fail(env, PCBENV_EINVAL, "null request");
    if (r->struct_size != (uint32_t)sizeof(pcbenv_visits_request)) return fail(env, PCBENV_EINVAL, "struct_size is not sizeof(pcbenv_visits_request)");
    if (r->logits_dtype != PCBENV_LOGITS_F32 && r->logits_dtype != PCBENV_LOGITS_BF16) return fail(env, PCBENV_EINVAL, "unknown logits dtype");
    CHECK_ACTION_FORMAT(env, r->action_format);
    if (r->num_targets < 1 || r->num_targets > PCBENV_MAX_TREE_CHILDREN) return fail(env, PCBENV_EINVAL, "num_targets must be in [1, 64]");
    if (r->num_rows < 0 || r->num_rows > INT32_MAX) return fail(env, PCBENV_EINVAL, "num_rows out of range");
    if (r->reserved != 0) return fail(env, PCBENV_EINVAL, "reserved must be 0");
    if (!r->logits || !r->mask_bits || !r->visits || !r->target_actions) return fail(env, PCBENV_EINVAL, "null logits, mask_bits, visits or target_actions");
    if (backward && (!r->stats || !r->grad_logits)) return fail(env, PCBENV_EINVAL, "null stats or grad_logits");
    const uintptr_t elem = r->logits_dtype == PCBENV_LOGITS_F32 ? 4 : 2;
    if ((uintptr_t)r->logits % elem != 0) return fail(env, PCBENV_EINVAL, "logits pointer not aligned to its element size");
    if ((uintptr_t)r->mask_bits % 8 != 0) return fail(env, PCBENV_EINVAL, "mask bits pointer not aligned to 8 bytes");
    if ((((uintptr_t)r->visits | (uintptr_t)r->target_actions) & 3u) != 0) return fail(env, PCBENV_EINVAL, "visits and target_actions must be 4-byte aligned");
    if ((uintptr_t)r->stats % 16 != 0) return fail(env, PCBENV_EINVAL, "stats pointer not aligned to 16 bytes");
    if (backward && (uintptr_t)r->grad_logits % elem != 0) return fail(env, PCBENV_EINVAL, "grad logits pointer not aligned to its element size");
    if (!env) return fail(0, PCBENV_EINVAL, "null handle");
    return PCBENV_OK;
}

VisitsArgs visits_args(const pcbenv_visits_request *r) {
    VisitsArgs a;
    a.logits = r->logits; a.mask_bits = (const u64 *)r->mask_bits; a.visits = r->visits; a.actions = r->target_actions;
    a.cross_entropy = r->cross_entropy; a.entropy = r->entropy; a.stats = r->stats; a.errors = (unsigned *)r->errors_dev;
    a.grad_ce = r->grad_cross_entropy; a.grad_entropy = r->grad_entropy; a.grad_logits = r->grad_logits;
    a.fmt = r->action_format; a.C = r->num_targets;
    return a;
}

}  // namespace

extern "C" int pcbenv_evaluate_visits(const pcbenv *cenv, const pcbenv_visits_request *r) {
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    if (const int rc = visits_checks(env, r, false)) return rc;
    if (r->num_rows == 0) return PCBENV_OK;
    DEVICE_GUARD(env);
    const DevParams &d = env->dp;
    const EvalGeom q{d.O, d.H, d.W, d.WW, (int)r->num_rows};
    const VisitsArgs a = visits_args(r);
    select_launch(r->logits_dtype, q.W, (uintptr_t)r->logits, q.O * q.H * q.W, PCB_VT_NW4_MIN_A, [&](auto t, auto vec, auto nw) {
        hipLaunchKernelGGL((k_evaluate_visits<typename decltype(t)::type, vec, nw>), dim3(q.rows), dim3(64 * nw), lds_bytes(q), (hipStream_t)r->stream, q, a);
    });
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}

// the gradient is stored with the same vectors as the logits are loaded: both pointers aligned
extern "C" int pcbenv_evaluate_visits_backward(const pcbenv *cenv, const pcbenv_visits_request *r) {
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    if (const int rc = visits_checks(env, r, true)) return rc;
    if (r->num_rows == 0) return PCBENV_OK;
    DEVICE_GUARD(env);
    const DevParams &d = env->dp;
    const EvalGeom q{d.O, d.H, d.W, d.WW, (int)r->num_rows};
    const VisitsArgs a = visits_args(r);
    const uintptr_t both = (uintptr_t)r->logits | (uintptr_t)r->grad_logits;
    select_launch(r->logits_dtype, q.W, both, q.O * q.H * q.W, PCB_VT_NW4_MIN_A, [&](auto t, auto vec, auto nw) {
        hipLaunchKernelGGL((k_evaluate_visits_backward<typename decltype(t)::type, vec, nw>), dim3(q.rows), dim3(64 * nw), backward_lds_bytes(q),
                           (hipStream_t)r->stream, q, a);
    });
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}
