// pcb_gumbel_leaves.h -- the SELECT of pcbenv_gumbel_advance_leaves (include/pcbenv_gumbel_leaves.h), stated once: L
// descents per launch of a tree whose root level is the Gumbel rule, for ONE root.  Plain C++17 that compiles alone, on the
// host and on the device, over pcb_gumbel.h (the root's scores, the counters, the table) and pcb_puct_leaves.h (pending
// visits, the score below the root, repeats), both of which stay as they are: k_gumbel_leaves (pcb_gumbel_leaves.hip)
// composes the pieces below with child c of the current node in lane c of a group, and tools/gumbel_leaves_check.cpp -- a CPU
// program -- composes them serially.  The other phases are the existing functions: pcb_gumbel.h:gumbel_begin and
// gumbel_choose, pcb_puct_leaves.h:leaves_absorb.  pcbenv/search.py:gumbel_search(leaves=L) is the specification.
//
// The scores of the root's children read visits and value_sum and never pending, and SELECT stores nothing to the tree but
// pending: they are computed once per launch.  What changes from leaf to leaf at the root is sim_index, which walks along
// the schedule, and sim_visits, which decides who is considered: a leaf commits both only when it was no repeat.
//
// The promise of pcb_puct.h holds here too: k and fc are compared with C and N before they address anything; sim_index
// addresses the table only while 0 <= t < n; pending, a table entry and a counter are data.
#pragma once
#include "pcb_gumbel.h"
#include "pcb_puct_leaves.h"

namespace pcb_gumbel_leaves {

using namespace pcb_puct_leaves;
using pcb_gumbel::best_at;
using pcb_gumbel::considered_candidates;
using pcb_gumbel::root_scores;
using pcb_gumbel::Rule;
using pcb_gumbel::scheduled;

// pcb_puct_leaves.h:leaves_descend's loop from level d at `node` on -- the levels above are the caller's, which has added
// their pending visits and written their path rows; a repeat takes those back as well (undo_pending walks d parents).
// Returns true if the descent was a repeat (nothing else is written then, and no pending visit stays).
PCB_TREE_HD inline bool descend_from(const Root &r, int *pending, int rows, int row, double c_puct, double lo, double hi, int node, int d, int *paths,
                                     int *path_len, int *selected, unsigned *err) {
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

// considered [Mc + 1, n]; sim_index: this root's element; sim_visits [C]: its row; pending [N]: its row; selected, path_len
// [P * L], paths [T, P * L, 3]: the whole tensors.  At most T levels per leaf.
PCB_TREE_HD inline unsigned gumbel_leaves_select(const Root &r, const Rule &q, int *pending, int L, const int *considered, int *sim_index,
                                                 int *sim_visits, int *paths, int *path_len, int *selected) {
    unsigned err = 0u;
    const int rows = r.P * L, row0 = leaf_row(r.p, L, 0);
    const int k = r.num_children[0], fc = r.first_child[0];
    const double lo = *r.lo, hi = *r.hi;
    const bool halts = stops(r.terminal[0], k);
    int l = 0;
    if (halts || !children_ok(fc, k, r.N, r.C) || *sim_index < 0) {  // no descent: the root itself, once
        if (!halts) err |= ERR_TREE;
        pending[0] = one_more(pending[0]);
        selected[row0] = 0;
        path_len[row0] = 0;
        l = 1;
    } else {
        double s[MAX_CHILDREN], x[MAX_CHILDREN];
        root_scores(r, q, k, fc, s, x);  // once: no leaf changes what they read
        const long long table_row = (long long)considered_candidates(q.Mc, k) * q.n;
        for (; l < L; l++) {
            const int t = *sim_index, row = row0 + l;
            if (!scheduled(t, q.n)) {  // out of budget: one descent by the pending-visit score from the root, and no more
                if (l > 0 || leaves_descend(r, pending, rows, row, q.c_puct, lo, hi, paths, path_len, selected, &err)) break;
                continue;
            }
            const int c = best_at(s, sim_visits, k, considered[table_row + t]);
            pending[0] = one_more(pending[0]);
            for (int i = 0; i < 3; i++) paths[step_major(0, rows, row, i)] = r.node_action[3 * (fc + c) + i];
            if (descend_from(r, pending, rows, row, q.c_puct, lo, hi, fc + c, 1, paths, path_len, selected, &err)) break;
            sim_visits[c] = pcb_gumbel::one_more(sim_visits[c]);  // a repeat does not get here: it consumes no simulation
            *sim_index = t + 1;
        }
    }
    for (; l < L; l++) { selected[leaf_row(r.p, L, l)] = -1; path_len[leaf_row(r.p, L, l)] = -1; }
    return err;
}

}  // namespace pcb_gumbel_leaves
