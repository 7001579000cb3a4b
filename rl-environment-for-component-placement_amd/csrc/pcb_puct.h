// pcb_puct.h -- the tree step of pcbenv_puct_advance, stated once: initialisation, PUCT selection, and the expansion and
// backup of one evaluation, for ONE root.  Plain C++17 that compiles alone, on the host and on the device: k_puct_advance
// (pcb_puct.hip) composes the pieces below with the children of a node spread over a group of lanes, and
// tools/puct_model_check.cpp -- a CPU program that replays recorded searches of pcbenv/search.py:puct_search, the
// specification -- composes them serially (puct_init, puct_select, puct_absorb).  One IEEE operation per written operator
// (the build passes -ffp-contract=off); no logarithm anywhere, so no table.
//
// The tree of root p lives in the caller's tensors, root-major, N node slots per root:
//   num_nodes [P] | parent, depth, visits, num_children, first_child [P, N] | node_action [P, N, 3]
//   prior, value_sum, value_max [P, N] float64 | terminal [P, N] uint8 | reward_lo, reward_hi [P] float64
// Slot 0 is the root.  A node is expanded once, with all its k <= C children at once: they take the consecutive slots
// first_child .. first_child + k - 1, so the lanes of a group load the children's fields from adjacent addresses.
// Values are finite numbers; priors are used as given.
//
// The promise of pcb_tree.h holds here too: every slot number or count read back from memory is compared with N or C
// before it addresses anything.  A tree the caller has damaged stops that root's phase there and reports ERR_TREE, it
// never sends a store outside the tensors.
#pragma once
#include "pcb_tree.h"

namespace pcb_puct {

using pcb_tree::back_up;  // visits, value_sum and value_max of the node and every ancestor: at most T + 1 nodes
using pcb_tree::beats;
using pcb_tree::neg_inf;
using pcb_tree::root_of;
using pcb_tree::slot_ok;
using pcb_tree::step_major;
using pcb_tree::ERR_FULL;  // bit 0: the children of a node were due but do not fit into the free slots; none was made
using pcb_tree::ERR_TREE;  // bit 1: `selected`, num_nodes, a child range or a parent stored in the tree is out of range
using pcb_tree::MAX_CHILDREN;
using pcb_tree::PHASE_ABSORB;
using pcb_tree::PHASE_INIT;
using pcb_tree::PHASE_SELECT;

// One root's slabs (the pointers already at root p) and what addresses the step-major tensors.
struct Root {
    int N, C, T, P, p;
    int *num_nodes, *parent, *depth, *visits, *num_children, *first_child, *node_action;
    double *prior, *value_sum, *value_max;
    uint8_t *terminal;
    double *lo, *hi;
};
// Root p of a batch: `a` is a kernel's argument block, the tensors of all P roots under the names above.
template <class Args> PCB_TREE_HD inline Root root_of_group(const Args &a, int p, int T) {
    const long long s = (long long)p * a.N;
    return Root{a.N, a.C, T, a.P, p, a.num_nodes + p, a.parent + s, a.depth + s, a.visits + s, a.num_children + s, a.first_child + s,
                a.node_action + 3 * s, a.prior + s, a.value_sum + s, a.value_max + s, a.terminal + s, a.lo + p, a.hi + p};
}

// ---- init ----------------------------------------------------------------------------------------------------------
// What one node slot holds before it is used; slot 0 is the root and holds the same.
PCB_TREE_HD inline void init_slot(const Root &r, int s) {
    r.parent[s] = -1; r.depth[s] = 0; r.visits[s] = 0; r.num_children[s] = 0; r.first_child[s] = -1;
    r.node_action[3 * s] = 0; r.node_action[3 * s + 1] = 0; r.node_action[3 * s + 2] = 0;
    r.prior[s] = 0.0; r.value_sum[s] = 0.0; r.value_max[s] = neg_inf(); r.terminal[s] = 0;
}
PCB_TREE_HD inline void init_scalars(const Root &r) { *r.num_nodes = 1; *r.lo = HUGE_VAL; *r.hi = neg_inf(); }
PCB_TREE_HD inline void puct_init(const Root &r) {
    for (int s = 0; s < r.N; s++) init_slot(r, s);
    init_scalars(r);
}

// ---- select --------------------------------------------------------------------------------------------------------
// The descent stops at a node that is terminal or has not been expanded.
PCB_TREE_HD inline bool stops(int terminal, int num_children) { return terminal != 0 || num_children == 0; }
// the children first_child .. first_child + k - 1 of an expanded node are slots of the tree behind the root
PCB_TREE_HD inline bool children_ok(int first_child, int k, int N, int C) {
    return k >= 1 && k <= C && first_child >= 1 && first_child <= N - k;
}
PCB_TREE_HD inline int at_least_1(int n) { return n < 1 ? 1 : n; }
// q + c_puct * prior * sqrt(visits(node)) / (1 + visits(child)), q the child's mean value normalised by the root's value
// range, 0 for a child not yet visited
PCB_TREE_HD inline double puct_score(double value_sum_c, int visits_c, double prior_c, double lo, double hi, double c_puct, int visits_node) {
    const double n_c = (double)visits_c;
    const double q = (visits_c > 0 && hi > lo) ? (value_sum_c / n_c - lo) / (hi - lo) : 0.0;
    const double u = c_puct * prior_c * root_of((double)at_least_1(visits_node)) / (1.0 + n_c);
    return q + u;
}

// Writes rows d < *path_len of paths [T, P, 3] (the others are untouched), *path_len = the levels taken, and *selected.
// At most T levels: the loop is bounded by max_steps, not by data.
PCB_TREE_HD inline unsigned puct_select(const Root &r, double c_puct, int *paths, int *path_len, int *selected) {
    unsigned err = 0u;
    const double lo = *r.lo, hi = *r.hi;
    int node = 0, d = 0;
    for (; d < r.T; d++) {
        const int k = r.num_children[node], fc = r.first_child[node];
        if (stops(r.terminal[node], k)) break;
        if (!children_ok(fc, k, r.N, r.C)) { err |= ERR_TREE; break; }
        const int n_p = r.visits[node];
        int best_c = -1;
        double best = 0.0;
        for (int c = 0; c < k; c++) {
            const int ch = fc + c;
            const double s = puct_score(r.value_sum[ch], r.visits[ch], r.prior[ch], lo, hi, c_puct, n_p);
            if (best_c < 0 || beats(s, c, best, best_c)) { best = s; best_c = c; }
        }
        node = fc + best_c;
        for (int i = 0; i < 3; i++) paths[step_major(d, r.P, r.p, i)] = r.node_action[3 * node + i];
    }
    *selected = node;
    *path_len = d;
    return err;
}

// ---- absorb --------------------------------------------------------------------------------------------------------
// how many of the candidates given become children: an out-of-range count is data, not an error
PCB_TREE_HD inline int kept_candidates(int cand_count, int K, int C) {
    const int most = K < C ? K : C;
    return cand_count < 0 ? 0 : cand_count > most ? most : cand_count;
}
// a node is expanded once, and never when the episode is over at it
PCB_TREE_HD inline bool expands(int leaf_terminal, int num_children, int terminal) { return leaf_terminal == 0 && num_children == 0 && terminal == 0; }
// child c of `node` in slot first + c: the fields of the slot the expansion sets (INIT left the others as a new node has them)
PCB_TREE_HD inline void make_child(const Root &r, int node, int slot, int depth, const int *action, float prior) {
    r.parent[slot] = node; r.depth[slot] = depth + 1;
    r.node_action[3 * slot] = action[0]; r.node_action[3 * slot + 1] = action[1]; r.node_action[3 * slot + 2] = action[2];
    r.prior[slot] = (double)prior;
}
PCB_TREE_HD inline void link_children(const Root &r, int node, int first, int k) {
    r.first_child[node] = first; r.num_children[node] = k; *r.num_nodes = first + k;
}
// value, leaf_terminal, cand_count: what the caller found at `selected`; cand_actions [K, 3] and cand_prior [K]: this root's rows.
PCB_TREE_HD inline unsigned puct_absorb(const Root &r, int selected, double value, int leaf_terminal, int cand_count, int K,
                                        const int *cand_actions, const float *cand_prior) {
    const int count = *r.num_nodes;
    if (!slot_ok(selected, r.N) || count < 1 || count > r.N) return ERR_TREE;
    unsigned err = 0u;
    const int node = selected, depth = r.depth[node];
    if (leaf_terminal != 0) r.terminal[node] = 1;
    else if (expands(leaf_terminal, r.num_children[node], r.terminal[node])) {
        const int k = kept_candidates(cand_count, K, r.C);
        if (k > 0 && count + k <= r.N) {
            for (int c = 0; c < k; c++) make_child(r, node, count + c, depth, cand_actions + 3 * c, cand_prior[c]);
            link_children(r, node, count, k);
        } else if (k > 0) err |= ERR_FULL;
    }
    *r.lo = value < *r.lo ? value : *r.lo;
    *r.hi = value > *r.hi ? value : *r.hi;
    err |= back_up(r, node, value);
    return err;
}

}  // namespace pcb_puct
