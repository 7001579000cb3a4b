// pcb_tree.hip -- k_tree_advance and its entry point pcbenv_tree_advance: UCT selection, expansion and backup of a batch
// of search trees on the device (what pcbenv/search.py:tree_search does with some hundred tensor operations per
// iteration).  Part of libpcbenv.so (CDNA4 / gfx950 only); a translation unit of its own, host side included, so that
// nothing here can change the builds of the other kernels or of the other entry points.
//
// The step of one root is pcb_tree.h (tree_init, tree_select, tree_absorb: the text tools/tree_model_check.cpp replays on
// the CPU); the kernel composes the same pieces with a group of G lanes per root, G the power of two >= max(C, 4), so a
// wavefront carries 64 / G roots and a 256-thread workgroup 256 / G.  Groups share nothing: no LDS, no barrier, and a
// group whose root does not exist exits whole.
//   select   lane c of the group owns child slot c of the current node.  Per level two load round trips: the node's flags,
//            its visits and the lane's child slot together, then the child's visits and value_sum and ln[visits(node)]
//            together.  The group argmax (pcb_tree::beats: the lowest slot on ties) is a shuffle butterfly; the winner's
//            action is copied to the path row by lanes 0..2 while the next level's loads are already under way.
//   absorb   the lanes compare the drawn action with their child's; the first match is found by ballot.  Lane 0 makes the
//            child and walks the backup chain -- one round trip per level: a node's parent, visits, value_sum and
//            value_max are loaded together.  The best_actions copy is spread over the group.
//   init     the slots and the child entries of a root are contiguous: the lanes stride them.
// A later phase of one launch reads what an earlier one stored through other lanes of the same wavefront; a
// wavefront-scope fence between the phases keeps the compiler from moving those loads up.
#include <hip/hip_runtime.h>

#include "pcb_host.h"
#include "pcb_tree.h"

static_assert(PCBENV_TREE_INIT == pcb_tree::PHASE_INIT && PCBENV_TREE_ABSORB == pcb_tree::PHASE_ABSORB &&
              PCBENV_TREE_SELECT == pcb_tree::PHASE_SELECT && PCBENV_MAX_TREE_CHILDREN == pcb_tree::MAX_CHILDREN,
              "pcbenv.h and pcb_tree.h name the same phases");
static_assert(sizeof(pcbenv_tree_request) == 224 && offsetof(pcbenv_tree_request, stream) == 216, "pcbenv/_lib.py:PcbenvTreeRequest");

namespace {

using namespace pcb_tree;
constexpr int BLOCK = 256;

// what the kernel needs of a request
struct TreeArgs {
    int phases, P, N, C, T;
    double c_uct;
    const double *ln;
    int *num_nodes, *parent, *depth, *visits, *num_children, *node_action, *children;
    double *value_sum, *value_max;
    uint8_t *terminal;
    double *lo, *hi, *best_reward;
    int *best_length, *best_actions, *selected, *path_len, *paths;
    const double *reward;
    const int *length, *actions;
    unsigned *errors;
};

__device__ inline Root root_of_group(const TreeArgs &a, int p) {
    const long long s = (long long)p * a.N;
    return Root{a.N, a.C, a.T, a.P, p, a.num_nodes + p, a.parent + s, a.depth + s, a.visits + s, a.num_children + s,
                a.node_action + 3 * s, a.children + s * a.C, a.value_sum + s, a.value_max + s, a.terminal + s,
                a.lo + p, a.hi + p, a.best_reward + p, a.best_length + p, a.best_actions};
}

// the ballot of this lane's group, bit c = lane c of the group
template <int G> __device__ inline unsigned long long group_ballot(bool v, int base) {
    const unsigned long long b = __ballot(v);
    if constexpr (G == 64) return b;
    else return (b >> base) & ((1ull << G) - 1ull);
}

template <int G> __device__ inline void init_phase(const Root &r, int lane) {
    for (int s = lane; s < r.N; s += G) init_slot(r, s);
    const long long entries = (long long)r.N * r.C;
    for (long long i = lane; i < entries; i += G) r.children[i] = -1;
    if (lane == 0) init_scalars(r);
}

// tree_absorb, the children of the selected node over the lanes; returns the error bits (the same in every lane)
template <int G> __device__ inline unsigned absorb_phase(const Root &r, const TreeArgs &a, int lane, int base) {
    const int selected = a.selected[r.p], count = *r.num_nodes;
    if (!slot_ok(selected, r.N) || count < 1 || count > r.N) return ERR_TREE;
    unsigned err = 0u;
    const int node = selected, depth = r.depth[node], nch = r.num_children[node], term = r.terminal[node];
    const int length = a.length[r.p];
    const double reward = a.reward[r.p], best = *r.best_reward, lo = *r.lo, hi = *r.hi;
    const bool drew = drew_action(length, depth, term);
    const int row = drawn_row(depth, r.T);
    const int a0 = a.actions[step_major(row, r.P, r.p, 0)], a1 = a.actions[step_major(row, r.P, r.p, 1)], a2 = a.actions[step_major(row, r.P, r.p, 2)];
    int leaf = node;
    if (drew) {
        const bool mine = lane < r.C && lane < nch;
        const int ch = mine ? r.children[(long long)node * r.C + lane] : 0;
        const bool bad = mine && !slot_ok(ch, r.N);
        const bool match = mine && !bad && same_action(r.node_action, ch, a0, a1, a2);
        const unsigned long long bads = group_ballot<G>(bad, base), matches = group_ballot<G>(match, base);
        // as the serial walk: a match in a slot below the first bad one counts, nothing from it on does
        const unsigned long long before_bad = bads ? ((bads & (0ull - bads)) - 1ull) : ~0ull;
        const unsigned long long hits = matches & before_bad;
        if (hits) leaf = __shfl(ch, base + __builtin_ctzll(hits));
        else if (bads) err |= ERR_TREE;
        else if (nch >= 0 && nch < r.C) {
            if (count < r.N) {
                if (lane == 0) make_child(r, node, count, depth, nch, a0, a1, a2, length);
                leaf = count;
            } else err |= ERR_FULL;
        }
    }
    unsigned up = 0u;
    if (lane == 0) {
        *r.lo = reward < lo ? reward : lo;
        *r.hi = reward > hi ? reward : hi;
        up = back_up(r, leaf, reward);
    }
    err |= __shfl(up, base);
    if (reward > best) {
        if (lane == 0) { *r.best_reward = reward; *r.best_length = length; }
        const int ints = 3 * rows_to_copy(length, r.T);
        for (int i = lane; i < ints; i += G) {
            const long long at = step_major(i / 3, r.P, r.p, i % 3);
            r.best_actions[at] = a.actions[at];
        }
    }
    return err;
}

// tree_select, child slot c of the current node in lane c
template <int G> __device__ inline unsigned select_phase(const Root &r, const TreeArgs &a, int lane, int base) {
    unsigned err = 0u;
    const double lo = *r.lo, hi = *r.hi;
    int node = 0, d = 0;
    for (; d < r.T; d++) {
        const int term = r.terminal[node], nch = r.num_children[node], vis = r.visits[node];
        const bool mine = lane < r.C;
        const int ch = mine ? r.children[(long long)node * r.C + lane] : 0;
        if (stops(term, nch, r.C)) break;
        const bool bad = mine && !slot_ok(ch, r.N);
        if (group_ballot<G>(bad, base)) { err |= ERR_TREE; break; }
        const int n_p = at_least_1(vis);
        const double ln_p = a.ln[n_p > r.N ? r.N : n_p];
        double s = mine ? uct_score(r.value_sum[ch], r.visits[ch], lo, hi, a.c_uct, ln_p) : neg_inf();
        int c = mine ? lane : MAX_CHILDREN + lane;  // a lane without a child loses against any child, whatever its score
        #pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {
            const double so = __shfl_xor(s, o);
            const int co = __shfl_xor(c, o);
            const bool other = co < MAX_CHILDREN && (c >= MAX_CHILDREN || beats(so, co, s, c));
            s = other ? so : s;
            c = other ? co : c;
        }
        node = __shfl(ch, base + __shfl(c, base));  // lane 0's verdict: one node per group whatever the scores were
        if (lane < 3) a.paths[step_major(d, r.P, r.p, lane)] = r.node_action[3 * node + lane];
    }
    if (lane == 0) { a.selected[r.p] = node; a.path_len[r.p] = d; }
    return err;
}

template <int G> __global__ __launch_bounds__(BLOCK) void k_tree_advance(const TreeArgs a) {
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

// ---- pcbenv_tree_advance -----------------------------------------------------------------------------------------
// As pcbenv_playout_paths: every argument check before a device is touched, the null handle last; then one launch.
extern "C" int pcbenv_tree_advance(const pcbenv *cenv, const pcbenv_tree_request *q) {
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    if (!q) return fail(env, PCBENV_EINVAL, "null request");
    if (q->struct_size != (uint32_t)sizeof(pcbenv_tree_request)) return fail(env, PCBENV_EINVAL, "struct_size is not sizeof(pcbenv_tree_request)");
    const int ph = q->phases;
    const bool init = ph & PCBENV_TREE_INIT, absorb = ph & PCBENV_TREE_ABSORB, select = ph & PCBENV_TREE_SELECT;
    if (ph == 0 || (ph & ~(PCBENV_TREE_INIT | PCBENV_TREE_ABSORB | PCBENV_TREE_SELECT)) != 0) return fail(env, PCBENV_EINVAL, "phases must be a non-empty set of INIT, ABSORB, SELECT");
    if (init && absorb) return fail(env, PCBENV_EINVAL, "phases: INIT cannot be combined with ABSORB");
    if (q->num_roots < 0) return fail(env, PCBENV_EINVAL, "num_roots must not be negative");
    if (q->capacity < 1) return fail(env, PCBENV_EINVAL, "capacity must be at least 1");
    if (q->max_children < 1 || q->max_children > PCBENV_MAX_TREE_CHILDREN) return fail(env, PCBENV_EINVAL, "max_children must be in [1, 64]");
    if (q->max_steps < 1) return fail(env, PCBENV_EINVAL, "max_steps must be at least 1");
    if (!q->num_nodes || !q->parent || !q->depth || !q->visits || !q->num_children || !q->node_action || !q->children ||
        !q->value_sum || !q->value_max || !q->terminal || !q->reward_lo || !q->reward_hi) return fail(env, PCBENV_EINVAL, "null tree tensor");
    if ((init || absorb) && (!q->best_reward || !q->best_length)) return fail(env, PCBENV_EINVAL, "null tree tensor");
    if (absorb && !q->best_actions) return fail(env, PCBENV_EINVAL, "null tree tensor");
    if ((absorb || select) && !q->selected) return fail(env, PCBENV_EINVAL, "null selected");
    if (select && (!q->path_len || !q->paths)) return fail(env, PCBENV_EINVAL, "null path_len or paths with SELECT");
    if (select && !q->ln_dev) return fail(env, PCBENV_EINVAL, "null ln with SELECT");
    if (absorb && (!q->reward || !q->length || !q->actions)) return fail(env, PCBENV_EINVAL, "null reward, length or actions with ABSORB");
    const uintptr_t doubles = (uintptr_t)q->ln_dev | (uintptr_t)q->value_sum | (uintptr_t)q->value_max | (uintptr_t)q->reward_lo |
                              (uintptr_t)q->reward_hi | (uintptr_t)q->best_reward | (uintptr_t)q->reward;
    if ((doubles & 7u) != 0) return fail(env, PCBENV_EINVAL, "ln and the float64 tensors must be 8-byte aligned");
    if (!env) return fail(0, PCBENV_EINVAL, "null handle");
    if (q->num_roots == 0) return PCBENV_OK;
    DEVICE_GUARD(env);
    TreeArgs a;
    a.phases = ph; a.P = q->num_roots; a.N = q->capacity; a.C = q->max_children; a.T = q->max_steps;
    a.c_uct = q->c_uct; a.ln = q->ln_dev;
    a.num_nodes = q->num_nodes; a.parent = q->parent; a.depth = q->depth; a.visits = q->visits; a.num_children = q->num_children;
    a.node_action = q->node_action; a.children = q->children; a.value_sum = q->value_sum; a.value_max = q->value_max;
    a.terminal = q->terminal; a.lo = q->reward_lo; a.hi = q->reward_hi; a.best_reward = q->best_reward;
    a.best_length = q->best_length; a.best_actions = q->best_actions; a.selected = q->selected; a.path_len = q->path_len;
    a.paths = q->paths; a.reward = q->reward; a.length = q->length; a.actions = q->actions; a.errors = (unsigned *)q->errors_dev;
    const int G = group_lanes(a.C);
    const unsigned grid = (unsigned)(((long long)a.P + BLOCK / G - 1) / (BLOCK / G));
    hipStream_t s = (hipStream_t)q->stream;
    switch (G) {
    case 4: hipLaunchKernelGGL(k_tree_advance<4>, dim3(grid), dim3(BLOCK), 0, s, a); break;
    case 8: hipLaunchKernelGGL(k_tree_advance<8>, dim3(grid), dim3(BLOCK), 0, s, a); break;
    case 16: hipLaunchKernelGGL(k_tree_advance<16>, dim3(grid), dim3(BLOCK), 0, s, a); break;
    case 32: hipLaunchKernelGGL(k_tree_advance<32>, dim3(grid), dim3(BLOCK), 0, s, a); break;
    default: hipLaunchKernelGGL(k_tree_advance<64>, dim3(grid), dim3(BLOCK), 0, s, a); break;
    }
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}
