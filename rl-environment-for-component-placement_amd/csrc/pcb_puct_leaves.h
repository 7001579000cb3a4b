// pcb_puct_leaves.h -- the tree step of pcbenv_puct_advance_leaves, stated once: a PUCT search that selects L leaves per
// root before anything is evaluated (leaf-parallel selection with virtual visits), for ONE root.  Plain C++17 that
// compiles alone, on the host and on the device, built on the pieces of pcb_puct.h, which stays as it is: k_puct_leaves
// (pcb_puct_leaves.hip) composes the pieces below with the children of a node spread over a group of lanes, and
// tools/puct_leaves_check.cpp -- a CPU program that replays recorded searches of pcbenv/search.py:puct_search(leaves=L),
// the specification -- composes them serially (leaves_init, leaves_select, leaves_absorb).  One IEEE operation per
// written operator, evaluated left to right (the build passes -ffp-contract=off); no logarithm anywhere.
//
// The tree is pcb_puct.h's, with one tensor more: pending int32 [P, N], the visits selected but not yet absorbed.  The
// exchange tensors have a leaf extent, root-major: row r = p * L + l is leaf l of root p (the order of playout(k = L)),
//   selected, path_len [P * L] | paths [T, P * L, 3] | value, leaf_terminal, cand_count [P * L] | cand_actions
//   [P * L, K, 3] | cand_prior [P * L, K].
//
// SELECT descends L times, leaf after leaf.  A descent adds one pending visit to every node it passes, the root and the
// node it ends at included, and the next descent counts a pending visit as a visit that returned reward_lo: the score of a
// child is leaves_score below, which is puct_score bit for bit while nothing is pending.  A descent that ends at a node
// that is not terminal, has no children and has a pending visit already is a REPEAT: every later descent of this call
// would end there as well, so the selection of the root stops -- this and all later leaves get selected = path_len = -1,
// and the repeat leaves no pending visit behind.  ABSORB takes the leaves in the same order; it is puct_absorb per leaf,
// and takes the pending visit off every node of the backup chain.  After ABSORB has taken every leaf of a SELECT, pending
// is zero everywhere and the tree is one pcb_puct.h and pcb_puct_move.h take unchanged.
// A SELECT that follows a SELECT with no ABSORB between them adds to the pending visits that are there: the caller pairs
// every SELECT with the ABSORB of its leaves.
//
// The promise of pcb_puct.h holds unchanged: every slot number or count read back from memory is compared with N or C
// before it addresses anything.  pending is data: it is added to visit counts and never addresses anything, so whatever
// it holds no store leaves the tensors (its sums are formed in 64 bits and its updates wrap).
#pragma once
#include "pcb_puct.h"

namespace pcb_puct_leaves {

using namespace pcb_puct;
enum { MAX_LEAVES = 64 };

// row r of leaf l of root p, and the extent of the exchange tensors
PCB_TREE_HD inline int leaf_row(int p, int L, int l) { return p * L + l; }

// ---- init ----------------------------------------------------------------------------------------------------------
PCB_TREE_HD inline void leaves_init(const Root &r, int *pending) {
    puct_init(r);
    for (int s = 0; s < r.N; s++) pending[s] = 0;
}

// ---- select --------------------------------------------------------------------------------------------------------
PCB_TREE_HD inline long long with_pending(int visits, int pending) { return (long long)visits + (long long)pending; }
PCB_TREE_HD inline int one_more(int n) { return (int)((unsigned)n + 1u); }
PCB_TREE_HD inline int one_less(int n) { return (int)((unsigned)n - 1u); }
// puct_score with n_c = visits + pending of the child and of the node, and the child's mean value taken as if each pending
// visit had returned reward_lo (q = 0 after normalisation): q * visits / n_c.  The factor is exactly 1.0 with pending == 0.
PCB_TREE_HD inline double leaves_score(double value_sum_c, int visits_c, int pending_c, double prior_c, double lo, double hi, double c_puct,
                                       int visits_node, int pending_node) {
    const double n_c = (double)with_pending(visits_c, pending_c);
    const double q = (visits_c > 0 && hi > lo) ? ((value_sum_c / (double)visits_c - lo) / (hi - lo)) * ((double)visits_c / n_c) : 0.0;
    const long long n_p = with_pending(visits_node, pending_node);
    const double u = c_puct * prior_c * root_of((double)(n_p < 1 ? 1 : n_p)) / (1.0 + n_c);
    return q + u;
}
// a descent that ends here would end here again: the node is waiting for its evaluation
PCB_TREE_HD inline bool repeats(int terminal, int num_children, int pending) { return terminal == 0 && num_children == 0 && pending > 0; }
// Takes back the pending visits a repeat added on the d nodes above `node`, walking the parents: at most d nodes.
PCB_TREE_HD inline unsigned undo_pending(const Root &r, int *pending, int node, int d) {
    int cur = r.parent[node];
    for (int i = 0; i < d && cur >= 0; i++) {
        if (!slot_ok(cur, r.N)) return ERR_TREE;
        pending[cur] = one_less(pending[cur]);
        cur = r.parent[cur];
    }
    return 0u;
}

// One descent, leaf `row` of the P * L rows.  Writes rows d < the levels taken of paths [T, P * L, 3].  Returns true if
// the descent was a repeat (nothing else is written then, and no pending visit stays).
PCB_TREE_HD inline bool leaves_descend(const Root &r, int *pending, int rows, int row, double c_puct, double lo, double hi, int *paths,
                                       int *path_len, int *selected, unsigned *err) {
    int node = 0, d = 0;
    for (;; d++) {
        const int k = r.num_children[node], fc = r.first_child[node], pend = pending[node];
        if (d >= r.T || stops(r.terminal[node], k)) break;
        if (!children_ok(fc, k, r.N, r.C)) { *err |= ERR_TREE; break; }
        const int n_p = r.visits[node];
        int best_c = -1;
        double best = 0.0;
        for (int c = 0; c < k; c++) {
            const int ch = fc + c;
            const double s = leaves_score(r.value_sum[ch], r.visits[ch], pending[ch], r.prior[ch], lo, hi, c_puct, n_p, pend);
            if (best_c < 0 || beats(s, c, best, best_c)) { best = s; best_c = c; }
        }
        pending[node] = one_more(pend);
        node = fc + best_c;
        for (int i = 0; i < 3; i++) paths[step_major(d, rows, row, i)] = r.node_action[3 * node + i];
    }
    if (repeats(r.terminal[node], r.num_children[node], pending[node])) {
        *err |= undo_pending(r, pending, node, d);
        return true;
    }
    pending[node] = one_more(pending[node]);
    selected[row] = node;
    path_len[row] = d;
    return false;
}

// selected, path_len [P * L], paths [T, P * L, 3]: the whole tensors.  At most T levels per leaf.
PCB_TREE_HD inline unsigned leaves_select(const Root &r, int *pending, int L, double c_puct, int *paths, int *path_len, int *selected) {
    unsigned err = 0u;
    const double lo = *r.lo, hi = *r.hi;
    for (int l = 0; l < L; l++) {
        if (!leaves_descend(r, pending, r.P * L, leaf_row(r.p, L, l), c_puct, lo, hi, paths, path_len, selected, &err)) continue;
        for (; l < L; l++) { selected[leaf_row(r.p, L, l)] = -1; path_len[leaf_row(r.p, L, l)] = -1; }
    }
    return err;
}

// ---- absorb --------------------------------------------------------------------------------------------------------
// The pending visit taken off every node of the chain back_up (pcb_tree.h) walks: the same bound, the same checks, so the
// two walks pass the same nodes and stop at the same one.
PCB_TREE_HD inline void take_pending(const Root &r, int *pending, int leaf) {
    int cur = leaf;
    for (int i = 0; i <= r.T && cur >= 0 && slot_ok(cur, r.N); i++) {
        pending[cur] = one_less(pending[cur]);
        cur = r.parent[cur];
    }
}
// One leaf: exactly puct_absorb, then take_pending.  selected and num_nodes are in range (leaves_absorb has looked), so an
// ERR_TREE of puct_absorb comes from its backup, and the second walk stops where that one did.
PCB_TREE_HD inline unsigned leaves_absorb_one(const Root &r, int *pending, int selected, double value, int leaf_terminal, int cand_count, int K,
                                              const int *cand_actions, const float *cand_prior) {
    const unsigned err = puct_absorb(r, selected, value, leaf_terminal, cand_count, K, cand_actions, cand_prior);
    take_pending(r, pending, selected);
    return err;
}
// back_up and take_pending as ONE walk: what lane 0 of k_puct_leaves runs, where a second walk would be a second chain of
// dependent loads.  tests/test_puct_leaves_gpu.py holds it to the two walks above in every tensor after every call.
PCB_TREE_HD inline unsigned leaves_back_up(const Root &r, int *pending, int leaf, double value) {
    return back_up(r, leaf, value, [pending](int cur) { pending[cur] = one_less(pending[cur]); });
}
// The leaves in order.  selected == -1: the leaf is skipped and none of its inputs is read.  A leaf that reports ERR_TREE
// (selected outside [-1, N), num_nodes out of range, a parent out of range) ends the root's phase.
PCB_TREE_HD inline unsigned leaves_absorb(const Root &r, int *pending, int L, const int *selected, const double *value, const uint8_t *leaf_terminal,
                                          const int *cand_count, int K, const int *cand_actions, const float *cand_prior) {
    unsigned err = 0u;
    for (int l = 0; l < L; l++) {
        const long long row = leaf_row(r.p, L, l);
        if (selected[row] == -1) continue;
        const int count = *r.num_nodes;
        const unsigned e = slot_ok(selected[row], r.N) && count >= 1 && count <= r.N ? leaves_absorb_one(r, pending, selected[row], value[row], leaf_terminal[row], cand_count[row], K,
                                                                           cand_actions + 3 * row * K, cand_prior + row * K)
                                                                                     : ERR_TREE;
        err |= e;
        if (e & ERR_TREE) break;
    }
    return err;
}

}  // namespace pcb_puct_leaves
