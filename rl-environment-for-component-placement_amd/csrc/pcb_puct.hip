// pcb_puct.hip -- k_puct_advance and its entry point pcbenv_puct_advance (include/pcbenv_search.h): PUCT selection,
// expansion and backup of a batch of search trees on the device (what pcbenv/search.py:puct_search does with some
// hundred tensor operations per iteration).  Part of libpcbenv.so (CDNA4 / gfx950 only); a translation unit of its own,
// host side included, so that nothing here can change the builds of the other kernels or of the other entry points.
//
// The step of one root is pcb_puct.h (puct_init, puct_select, puct_absorb: the text tools/puct_model_check.cpp replays
// on the CPU); the kernel composes the same pieces with a group of G lanes per root, G the power of two >= max(C, 4), so
// a wavefront carries 64 / G roots and a 256-thread workgroup 256 / G.  Groups share nothing: no LDS, no barrier, and a
// group whose root does not exist exits whole.
//   select   lane c of the group owns child first_child + c of the current node.  Per level two load round trips: the
//            node's terminal, num_children, first_child and visits together, then the children's visits, value_sum and
//            prior -- consecutive slots, so a group's loads are contiguous; k_tree_advance has to gather them.  The group
//            argmax (pcb_tree::beats: the lowest child on ties) is a shuffle butterfly; the winner's action is copied to
//            the path row by lanes 0..2 while the next level's loads are already under way.
//   absorb   lanes c < k write one child slot each; lane 0 writes the node's fields and the scalars and walks the backup
//            chain -- one round trip per level: a node's parent, visits, value_sum and value_max are loaded together.
//   init     the slots of a root are contiguous: the lanes stride them.
// A later phase of one launch reads what an earlier one stored through other lanes of the same wavefront; a
// wavefront-scope fence between the phases keeps the compiler from moving those loads up.
#include <hip/hip_runtime.h>

#include "pcb_host.h"
#include "pcbenv_search.h"
#include "pcb_puct.h"

static_assert(PCBENV_TREE_INIT == pcb_puct::PHASE_INIT && PCBENV_TREE_ABSORB == pcb_puct::PHASE_ABSORB &&
              PCBENV_TREE_SELECT == pcb_puct::PHASE_SELECT && PCBENV_MAX_TREE_CHILDREN == pcb_puct::MAX_CHILDREN,
              "pcbenv.h and pcb_puct.h name the same phases");
static_assert(sizeof(pcbenv_puct_request) == 224 && offsetof(pcbenv_puct_request, stream) == 216, "pcbenv/_search_lib.py:PcbenvPuctRequest");

namespace {

using namespace pcb_puct;
constexpr int BLOCK = 256;

// what the kernel needs of a request
struct PuctArgs {
    int phases, P, N, C, T, K;
    double c_puct;
    int *num_nodes, *parent, *depth, *visits, *num_children, *first_child, *node_action;
    double *prior, *value_sum, *value_max;
    uint8_t *terminal;
    double *lo, *hi;
    int *selected, *path_len, *paths;
    const double *value;
    const uint8_t *leaf_terminal;
    const int *cand_count, *cand_actions;
    const float *cand_prior;
    unsigned *errors;
};

__device__ inline Root root_of_group(const PuctArgs &a, int p) {
    const long long s = (long long)p * a.N;
    return Root{a.N, a.C, a.T, a.P, p, a.num_nodes + p, a.parent + s, a.depth + s, a.visits + s, a.num_children + s, a.first_child + s,
                a.node_action + 3 * s, a.prior + s, a.value_sum + s, a.value_max + s, a.terminal + s, a.lo + p, a.hi + p};
}

template <int G> __device__ inline void init_phase(const Root &r, int lane) {
    for (int s = lane; s < r.N; s += G) init_slot(r, s);
    if (lane == 0) init_scalars(r);
}

// puct_absorb, the new children over the lanes; returns the error bits (the same in every lane)
template <int G> __device__ inline unsigned absorb_phase(const Root &r, const PuctArgs &a, int lane, int base) {
    const int selected = a.selected[r.p], count = *r.num_nodes;
    if (!slot_ok(selected, r.N) || count < 1 || count > r.N) return ERR_TREE;
    unsigned err = 0u;
    const int node = selected, depth = r.depth[node], nch = r.num_children[node], term = r.terminal[node];
    const int leaf_terminal = a.leaf_terminal[r.p], cand_count = a.cand_count[r.p];
    const double value = a.value[r.p], lo = *r.lo, hi = *r.hi;
    if (leaf_terminal != 0) {
        if (lane == 0) r.terminal[node] = 1;
    } else if (expands(leaf_terminal, nch, term)) {
        const int k = kept_candidates(cand_count, a.K, r.C);
        if (k > 0 && count + k <= r.N) {
            const long long row = (long long)r.p * a.K;
            if (lane < k) make_child(r, node, count + lane, depth, a.cand_actions + 3 * (row + lane), a.cand_prior[row + lane]);
            if (lane == 0) link_children(r, node, count, k);
        } else if (k > 0) err |= ERR_FULL;
    }
    unsigned up = 0u;
    if (lane == 0) {
        *r.lo = value < lo ? value : lo;
        *r.hi = value > hi ? value : hi;
        up = back_up(r, node, value);
    }
    err |= __shfl(up, base);
    return err;
}

// puct_select, child first_child + c of the current node in lane c
template <int G> __device__ inline unsigned select_phase(const Root &r, const PuctArgs &a, int lane, int base) {
    unsigned err = 0u;
    const double lo = *r.lo, hi = *r.hi;
    int node = 0, d = 0;
    for (; d < r.T; d++) {
        const int term = r.terminal[node], k = r.num_children[node], fc = r.first_child[node], vis = r.visits[node];
        if (stops(term, k)) break;
        if (!children_ok(fc, k, r.N, r.C)) { err |= ERR_TREE; break; }
        const bool mine = lane < k;
        const int ch = fc + (mine ? lane : 0);
        double s = mine ? puct_score(r.value_sum[ch], r.visits[ch], r.prior[ch], lo, hi, a.c_puct, vis) : neg_inf();
        int c = mine ? lane : MAX_CHILDREN + lane;  // a lane without a child loses against any child, whatever its score
        #pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {
            const double so = __shfl_xor(s, o);
            const int co = __shfl_xor(c, o);
            const bool other = co < MAX_CHILDREN && (c >= MAX_CHILDREN || beats(so, co, s, c));
            s = other ? so : s;
            c = other ? co : c;
        }
        node = fc + __shfl(c, base);  // lane 0's verdict: one node per group whatever the scores were
        if (lane < 3) a.paths[step_major(d, r.P, r.p, lane)] = r.node_action[3 * node + lane];
    }
    if (lane == 0) { a.selected[r.p] = node; a.path_len[r.p] = d; }
    return err;
}

template <int G> __global__ __launch_bounds__(BLOCK) void k_puct_advance(const PuctArgs a) {
    static_assert(G >= 4 && G <= 64 && (G & (G - 1)) == 0, "a group is a power-of-two part of a wavefront");
    const unsigned p = blockIdx.x * (BLOCK / G) + threadIdx.x / G;
    if (p >= (unsigned)a.P) return;
    const int lane = threadIdx.x % G, base = (threadIdx.x & 63) - lane;
    const Root r = root_of_group(a, (int)p);
    unsigned err = 0u;
    if (a.phases & PHASE_INIT) {
        init_phase<G>(r, lane);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    if (a.phases & PHASE_ABSORB) {
        err |= absorb_phase<G>(r, a, lane, base);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    if (a.phases & PHASE_SELECT) err |= select_phase<G>(r, a, lane, base);
    if (err != 0u && lane == 0 && a.errors) atomicOr(a.errors, err);
}

int group_lanes(int C) { int g = 4; while (g < C) g <<= 1; return g; }

}  // namespace

// ---- pcbenv_puct_advance -----------------------------------------------------------------------------------------
// As pcbenv_tree_advance: every argument check before a device is touched, the null handle last; then one launch.
extern "C" int pcbenv_puct_advance(const pcbenv *cenv, const pcbenv_puct_request *q) {
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    if (!q) return fail(env, PCBENV_EINVAL, "null request");
    if (q->struct_size != (uint32_t)sizeof(pcbenv_puct_request)) return fail(env, PCBENV_EINVAL, "struct_size is not sizeof(pcbenv_puct_request)");
    const int ph = q->phases;
    const bool init = ph & PCBENV_TREE_INIT, absorb = ph & PCBENV_TREE_ABSORB, select = ph & PCBENV_TREE_SELECT;
    if (ph == 0 || (ph & ~(PCBENV_TREE_INIT | PCBENV_TREE_ABSORB | PCBENV_TREE_SELECT)) != 0) return fail(env, PCBENV_EINVAL, "phases must be a non-empty set of INIT, ABSORB, SELECT");
    if (init && absorb) return fail(env, PCBENV_EINVAL, "phases: INIT cannot be combined with ABSORB");
    if (q->num_roots < 0) return fail(env, PCBENV_EINVAL, "num_roots must not be negative");
    if (q->capacity < 1) return fail(env, PCBENV_EINVAL, "capacity must be at least 1");
    if (q->max_children < 1 || q->max_children > PCBENV_MAX_TREE_CHILDREN) return fail(env, PCBENV_EINVAL, "max_children must be in [1, 64]");
    if (q->max_steps < 1) return fail(env, PCBENV_EINVAL, "max_steps must be at least 1");
    if (absorb && q->num_candidates < 1) return fail(env, PCBENV_EINVAL, "num_candidates must be at least 1 with ABSORB");
    if (q->reserved != 0) return fail(env, PCBENV_EINVAL, "reserved must be 0");
    if (!q->num_nodes || !q->parent || !q->depth || !q->visits || !q->num_children || !q->first_child || !q->node_action || !q->prior ||
        !q->value_sum || !q->value_max || !q->terminal || !q->reward_lo || !q->reward_hi) return fail(env, PCBENV_EINVAL, "null tree tensor");
    if ((absorb || select) && !q->selected) return fail(env, PCBENV_EINVAL, "null selected");
    if (select && (!q->path_len || !q->paths)) return fail(env, PCBENV_EINVAL, "null path_len or paths with SELECT");
    if (absorb && (!q->value || !q->leaf_terminal || !q->cand_count || !q->cand_actions || !q->cand_prior))
        return fail(env, PCBENV_EINVAL, "null value, leaf_terminal, cand_count, cand_actions or cand_prior with ABSORB");
    const uintptr_t doubles = (uintptr_t)q->prior | (uintptr_t)q->value_sum | (uintptr_t)q->value_max | (uintptr_t)q->reward_lo |
                              (uintptr_t)q->reward_hi | (absorb ? (uintptr_t)q->value : 0);
    if ((doubles & 7u) != 0) return fail(env, PCBENV_EINVAL, "the float64 tensors must be 8-byte aligned");
    if (absorb && ((uintptr_t)q->cand_prior & 3u) != 0) return fail(env, PCBENV_EINVAL, "cand_prior must be 4-byte aligned");
    if (!env) return fail(0, PCBENV_EINVAL, "null handle");
    if (q->num_roots == 0) return PCBENV_OK;
    DEVICE_GUARD(env);
    PuctArgs a;
    a.phases = ph; a.P = q->num_roots; a.N = q->capacity; a.C = q->max_children; a.T = q->max_steps; a.K = q->num_candidates;
    a.c_puct = q->c_puct;
    a.num_nodes = q->num_nodes; a.parent = q->parent; a.depth = q->depth; a.visits = q->visits; a.num_children = q->num_children;
    a.first_child = q->first_child; a.node_action = q->node_action; a.prior = q->prior; a.value_sum = q->value_sum; a.value_max = q->value_max;
    a.terminal = q->terminal; a.lo = q->reward_lo; a.hi = q->reward_hi; a.selected = q->selected; a.path_len = q->path_len;
    a.paths = q->paths; a.value = q->value; a.leaf_terminal = q->leaf_terminal; a.cand_count = q->cand_count; a.cand_actions = q->cand_actions;
    a.cand_prior = q->cand_prior; a.errors = (unsigned *)q->errors_dev;
    const int G = group_lanes(a.C);
    const unsigned grid = (unsigned)(((long long)a.P + BLOCK / G - 1) / (BLOCK / G));
    hipStream_t s = (hipStream_t)q->stream;
    switch (G) {
    case 4: hipLaunchKernelGGL(k_puct_advance<4>, dim3(grid), dim3(BLOCK), 0, s, a); break;
    case 8: hipLaunchKernelGGL(k_puct_advance<8>, dim3(grid), dim3(BLOCK), 0, s, a); break;
    case 16: hipLaunchKernelGGL(k_puct_advance<16>, dim3(grid), dim3(BLOCK), 0, s, a); break;
    case 32: hipLaunchKernelGGL(k_puct_advance<32>, dim3(grid), dim3(BLOCK), 0, s, a); break;
    default: hipLaunchKernelGGL(k_puct_advance<64>, dim3(grid), dim3(BLOCK), 0, s, a); break;
    }
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}
