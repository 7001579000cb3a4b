// pcb_tree.h -- the tree step of pcbenv_tree_advance, stated once: initialisation, UCT selection, and the expansion and
// backup of one playout, for ONE root.  Plain C++17 that compiles alone, on the host and on the device: k_tree_advance
// (pcb_tree.hip) composes the pieces below with the children of a node spread over a group of lanes, and
// tools/tree_model_check.cpp -- a CPU program that replays recorded searches of pcbenv/search.py:tree_search, the
// specification -- composes them serially (tree_init, tree_select, tree_absorb).  One IEEE operation per written operator
// (the build passes -ffp-contract=off); no call of log: ln n comes from the caller's table.
//
// The tree of root p lives in the caller's tensors, root-major, N node slots per root, C child slots per node:
//   num_nodes [P] | parent, depth, visits, num_children [P, N] | node_action [P, N, 3] | children [P, N, C]
//   value_sum, value_max [P, N] float64 | terminal [P, N] uint8 | reward_lo, reward_hi, best_reward [P] float64
//   best_length [P] | best_actions [T, P, 3] (step-major, as the playout writes its actions)
// Slot 0 is the root; slots are filled in the order the nodes are made.  Rewards are finite numbers.
//
// Every slot number read back from memory is compared with N before it addresses anything: a tree the caller has
// damaged stops the walk there and reports ERR_TREE, it never sends a store outside the tensors.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCB_TREE_HD __host__ __device__
#else
#define PCB_TREE_HD
#endif

namespace pcb_tree {

enum { PHASE_INIT = 1, PHASE_ABSORB = 2, PHASE_SELECT = 4, MAX_CHILDREN = 64 };
enum : unsigned { ERR_FULL = 1u,    // bit 0: a child was due but all N slots are in use; the playout went into the selected node
                  ERR_TREE = 2u };  // bit 1: `selected`, num_nodes or a slot number stored in the tree is out of range

// One root's slabs (the pointers already at root p) and what addresses the step-major tensors.
struct Root {
    int N, C, T, P, p;
    int *num_nodes, *parent, *depth, *visits, *num_children, *node_action, *children;
    double *value_sum, *value_max;
    uint8_t *terminal;
    double *lo, *hi, *best_reward;
    int *best_length, *best_actions;  // best_actions: the base of [T, P, 3]
};
// element k of row t of a step-major [T, P, 3] tensor, for root p
PCB_TREE_HD inline long long step_major(int t, int P, int p, int k) { return ((long long)t * P + p) * 3 + k; }
PCB_TREE_HD inline bool slot_ok(int s, int N) { return (unsigned)s < (unsigned)N; }
PCB_TREE_HD inline double neg_inf() { return -HUGE_VAL; }
PCB_TREE_HD inline double root_of(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(x);
#else
    return sqrt(x);
#endif
}

// ---- init ----------------------------------------------------------------------------------------------------------
// What one node slot and one child entry hold before they are used; slot 0 is the root and holds the same.
PCB_TREE_HD inline void init_slot(const Root &r, int s) {
    r.parent[s] = -1; r.depth[s] = 0; r.visits[s] = 0; r.num_children[s] = 0;
    r.value_sum[s] = 0.0; r.value_max[s] = neg_inf(); r.terminal[s] = 0;
    r.node_action[3 * s] = 0; r.node_action[3 * s + 1] = 0; r.node_action[3 * s + 2] = 0;
}
PCB_TREE_HD inline void init_scalars(const Root &r) {
    *r.num_nodes = 1; *r.lo = HUGE_VAL; *r.hi = neg_inf(); *r.best_reward = neg_inf(); *r.best_length = 0;
}
PCB_TREE_HD inline void tree_init(const Root &r) {
    for (int s = 0; s < r.N; s++) init_slot(r, s);
    for (long long i = 0; i < (long long)r.N * r.C; i++) r.children[i] = -1;
    init_scalars(r);
}

// ---- select --------------------------------------------------------------------------------------------------------
// The descent stops at a node that is terminal or has a free child slot.
PCB_TREE_HD inline bool stops(int terminal, int num_children, int C) { return terminal != 0 || num_children < C; }
PCB_TREE_HD inline int at_least_1(int n) { return n < 1 ? 1 : n; }
// q + c_uct * sqrt(ln[visits(node)] / visits(child)), q the child's mean reward normalised by the root's reward range
PCB_TREE_HD inline double uct_score(double value_sum_c, int visits_c, double lo, double hi, double c_uct, double ln_parent) {
    const double n_c = (double)at_least_1(visits_c);
    const double mean = value_sum_c / n_c;
    const double q = hi > lo ? (mean - lo) / (hi - lo) : 0.0;
    return q + c_uct * root_of(ln_parent / n_c);
}
// (score b, slot b) beats (score a, slot a): the first maximum wins, so an equal score in a higher slot does not
PCB_TREE_HD inline bool beats(double sb, int cb, double sa, int ca) { return sb > sa || (sb == sa && cb < ca); }

// Writes rows d < *path_len of paths [T, P, 3] (the others are untouched), *path_len = the levels taken = depth(selected),
// and *selected.  ln: [N + 1], ln[n] = the caller's ln n.  At most T levels: the loop is bounded by max_steps, not by data.
PCB_TREE_HD inline unsigned tree_select(const Root &r, double c_uct, const double *ln, int *paths, int *path_len, int *selected) {
    unsigned err = 0u;
    const double lo = *r.lo, hi = *r.hi;
    int node = 0, d = 0;
    for (; d < r.T; d++) {
        if (stops(r.terminal[node], r.num_children[node], r.C)) break;
        const int n_p = at_least_1(r.visits[node]);
        const double ln_p = ln[n_p > r.N ? r.N : n_p];
        int best_c = -1, best_slot = -1;
        double best = 0.0;
        for (int c = 0; c < r.C; c++) {
            const int ch = r.children[(long long)node * r.C + c];
            if (!slot_ok(ch, r.N)) { err |= ERR_TREE; best_c = -1; break; }
            const double s = uct_score(r.value_sum[ch], r.visits[ch], lo, hi, c_uct, ln_p);
            if (best_c < 0 || beats(s, c, best, best_c)) { best = s; best_c = c; best_slot = ch; }
        }
        if (best_c < 0) break;
        node = best_slot;
        for (int k = 0; k < 3; k++) paths[step_major(d, r.P, r.p, k)] = r.node_action[3 * node + k];
    }
    *selected = node;
    *path_len = d;
    return err;
}

// ---- absorb --------------------------------------------------------------------------------------------------------
// The playout from `selected` drew an action of its own iff it outlived the path and the node is not terminal.
PCB_TREE_HD inline bool drew_action(int length, int depth, int terminal) { return length > depth && terminal == 0; }
// the row of the playout's actions that holds it
PCB_TREE_HD inline int drawn_row(int depth, int T) { return depth < 0 ? 0 : depth > T - 1 ? T - 1 : depth; }
PCB_TREE_HD inline bool same_action(const int *node_action, int s, int a0, int a1, int a2) {
    return node_action[3 * s] == a0 && node_action[3 * s + 1] == a1 && node_action[3 * s + 2] == a2;
}
// A new child of `node` in slot `slot` (= num_nodes): the fields of the slot, the parent's child list, the counts.
PCB_TREE_HD inline void make_child(const Root &r, int node, int slot, int depth, int nch, int a0, int a1, int a2, int length) {
    r.parent[slot] = node; r.depth[slot] = depth + 1;
    r.node_action[3 * slot] = a0; r.node_action[3 * slot + 1] = a1; r.node_action[3 * slot + 2] = a2;
    r.terminal[slot] = length <= depth + 1 ? 1 : 0;
    r.children[(long long)node * r.C + nch] = slot;
    r.num_children[node] = nch + 1;
    *r.num_nodes = slot + 1;
}
// visits, value_sum and value_max of the leaf and every ancestor: at most T + 1 nodes.  The one backup walk of every tree
// here (R: this Root or pcb_puct.h's); also(cur): what else the walk does at a node (pcb_puct_leaves.h: its pending visit).
template <class R, class Also> PCB_TREE_HD inline unsigned back_up(const R &r, int leaf, double reward, Also also) {
    int cur = leaf;
    for (int i = 0; i <= r.T && cur >= 0; i++) {
        if (!slot_ok(cur, r.N)) return ERR_TREE;
        const int up = r.parent[cur];
        r.visits[cur] = r.visits[cur] + 1;
        r.value_sum[cur] = r.value_sum[cur] + reward;
        r.value_max[cur] = reward > r.value_max[cur] ? reward : r.value_max[cur];
        also(cur);
        cur = up;
    }
    return 0u;
}
template <class R> PCB_TREE_HD inline unsigned back_up(const R &r, int leaf, double reward) { return back_up(r, leaf, reward, [](int) {}); }
PCB_TREE_HD inline int rows_to_copy(int length, int T) { return length < 0 ? 0 : length > T ? T : length; }

// reward, length, actions [T, P, 3]: what the playout from `selected` returned for this root.
PCB_TREE_HD inline unsigned tree_absorb(const Root &r, int selected, double reward, int length, const int *actions) {
    const int count = *r.num_nodes;
    if (!slot_ok(selected, r.N) || count < 1 || count > r.N) return ERR_TREE;
    unsigned err = 0u;
    const int node = selected, depth = r.depth[node], nch = r.num_children[node];
    const bool drew = drew_action(length, depth, r.terminal[node]);
    const int row = drawn_row(depth, r.T);
    const int a0 = actions[step_major(row, r.P, r.p, 0)], a1 = actions[step_major(row, r.P, r.p, 1)], a2 = actions[step_major(row, r.P, r.p, 2)];
    int leaf = node;
    bool found = false;
    if (drew) {
        for (int c = 0; c < r.C && c < nch && !found; c++) {
            const int ch = r.children[(long long)node * r.C + c];
            if (!slot_ok(ch, r.N)) { err |= ERR_TREE; break; }
            if (same_action(r.node_action, ch, a0, a1, a2)) { leaf = ch; found = true; }
        }
        if (!found && err == 0u && nch >= 0 && nch < r.C) {
            if (count < r.N) { make_child(r, node, count, depth, nch, a0, a1, a2, length); leaf = count; }
            else err |= ERR_FULL;
        }
    }
    *r.lo = reward < *r.lo ? reward : *r.lo;
    *r.hi = reward > *r.hi ? reward : *r.hi;
    err |= back_up(r, leaf, reward);
    if (reward > *r.best_reward) {
        *r.best_reward = reward; *r.best_length = length;
        const int rows = rows_to_copy(length, r.T);
        for (int t = 0; t < rows; t++)
            for (int k = 0; k < 3; k++) r.best_actions[step_major(t, r.P, r.p, k)] = actions[step_major(t, r.P, r.p, k)];
    }
    return err;
}

}  // namespace pcb_tree
