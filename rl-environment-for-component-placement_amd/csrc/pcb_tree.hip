// pcb_tree.hip -- k_tree_advance and its entry point pcbenv_tree_advance: UCT selection, expansion and backup of a batch
// of search trees on the device (what pcbenv/search.py:tree_search does with some hundred tensor operations per
// iteration).  Part of libpcbenv.so (CDNA4 / gfx950 only); a translation unit of its own, host side included, so that
// nothing here can change the builds of the other kernels or of the other entry points.
//
// The step of one root is pcb_tree.h (tree_init, tree_select, tree_absorb: the text tools/tree_model_check.cpp replays on
// the CPU); the kernel composes the same pieces with a group of G lanes per root: the mapping, the phases and the fence
// between them are pcb_group.h's.  What a lane loads and stores:
//   select   lane c of the group owns child slot c of the current node.  Per level two load round trips: the node's flags,
//            its visits and the lane's child slot together, then the child's visits and value_sum and ln[visits(node)]
//            together.  The group argmax (pcb_tree::beats: the lowest slot on ties) is a shuffle butterfly; the winner's
//            action is copied to the path row by lanes 0..2 while the next level's loads are already under way.
//   absorb   the lanes compare the drawn action with their child's; the first match is found by ballot.  Lane 0 makes the
//            child and walks the backup chain -- one round trip per level: a node's parent, visits, value_sum and
//            value_max are loaded together.  The best_actions copy is spread over the group.
//   init     the slots and the child entries of a root are contiguous: the lanes stride them.
#include <hip/hip_runtime.h>

#include "pcb_group.h"
#include "pcb_tree_host.h"

static_assert(PCBENV_TREE_INIT == pcb_tree::PHASE_INIT && PCBENV_TREE_ABSORB == pcb_tree::PHASE_ABSORB &&
              PCBENV_TREE_SELECT == pcb_tree::PHASE_SELECT && PCBENV_MAX_TREE_CHILDREN == pcb_tree::MAX_CHILDREN,
              "pcbenv.h and pcb_tree.h name the same phases");
static_assert(sizeof(pcbenv_tree_request) == 224 && offsetof(pcbenv_tree_request, stream) == 216, "pcbenv/_lib.py:PcbenvTreeRequest");

namespace {

using namespace pcb_tree;
using pcb_group::BLOCK;
using pcb_group::group_ballot;

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
        PCB_GROUP_ARGMAX(G, mine, lane, s, c, beats)
        node = __shfl(ch, base + __shfl(c, base));  // lane 0's verdict: one node per group whatever the scores were
        if (lane < 3) a.paths[step_major(d, r.P, r.p, lane)] = r.node_action[3 * node + lane];
    }
    if (lane == 0) { a.selected[r.p] = node; a.path_len[r.p] = d; }
    return err;
}

template <int G> __global__ __launch_bounds__(BLOCK) void k_tree_advance(const TreeArgs a) {
    PCB_GROUP_ENTER(G, a);
    const Root r = root_of_group(a, (int)p);
    PCB_GROUP_PHASES(a, init_phase<G>(r, lane), absorb_phase<G>(r, a, lane, base), select_phase<G>(r, a, lane, base));
}

}  // namespace

// ---- pcbenv_tree_advance -----------------------------------------------------------------------------------------
// As pcbenv_playout_paths: every argument check before a device is touched, the null handle last; then one launch.
extern "C" int pcbenv_tree_advance(const pcbenv *cenv, const pcbenv_tree_request *q) {
    using namespace pcb_tree_host;
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    PCB_TRY(check_search_request(env, q, "pcbenv_tree_request"));
    const Phases ph = phases_of(q->phases);
    if (!q->num_nodes || !q->parent || !q->depth || !q->visits || !q->num_children || !q->node_action || !q->children ||
        !q->value_sum || !q->value_max || !q->terminal || !q->reward_lo || !q->reward_hi) return fail(env, PCBENV_EINVAL, "null tree tensor");
    if ((ph.init || ph.absorb) && (!q->best_reward || !q->best_length)) return fail(env, PCBENV_EINVAL, "null tree tensor");
    if (ph.absorb && !q->best_actions) return fail(env, PCBENV_EINVAL, "null tree tensor");
    PCB_TRY(check_exchange(env, q, ph));
    if (ph.select && !q->ln_dev) return fail(env, PCBENV_EINVAL, "null ln with SELECT");
    if (ph.absorb && (!q->reward || !q->length || !q->actions)) return fail(env, PCBENV_EINVAL, "null reward, length or actions with ABSORB");
    const uintptr_t doubles = (uintptr_t)q->ln_dev | (uintptr_t)q->value_sum | (uintptr_t)q->value_max | (uintptr_t)q->reward_lo |
                              (uintptr_t)q->reward_hi | (uintptr_t)q->best_reward | (uintptr_t)q->reward;
    if ((doubles & 7u) != 0) return fail(env, PCBENV_EINVAL, "ln and the float64 tensors must be 8-byte aligned");
    PCB_TREE_CHECKS_END(env, q);
    TreeArgs a;
    a.phases = q->phases; a.P = q->num_roots; a.N = q->capacity; a.C = q->max_children; a.T = q->max_steps;
    a.c_uct = q->c_uct; a.ln = q->ln_dev;
    a.num_nodes = q->num_nodes; a.parent = q->parent; a.depth = q->depth; a.visits = q->visits; a.num_children = q->num_children;
    a.node_action = q->node_action; a.children = q->children; a.value_sum = q->value_sum; a.value_max = q->value_max;
    a.terminal = q->terminal; a.lo = q->reward_lo; a.hi = q->reward_hi; a.best_reward = q->best_reward;
    a.best_length = q->best_length; a.best_actions = q->best_actions; a.selected = q->selected; a.path_len = q->path_len;
    a.paths = q->paths; a.reward = q->reward; a.length = q->length; a.actions = q->actions; a.errors = (unsigned *)q->errors_dev;
    PCB_GROUP_LAUNCH(k_tree_advance, a, (hipStream_t)q->stream);
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}
