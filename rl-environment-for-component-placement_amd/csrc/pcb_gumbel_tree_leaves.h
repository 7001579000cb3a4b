// pcb_gumbel_tree_leaves.h -- the SELECT of pcbenv_gumbel_tree_advance_leaves (include/pcbenv_gumbel_tree_leaves.h), stated
// once: L descents per launch of a tree under the full Gumbel rule, for ONE root.  Plain C++17 that compiles alone, on the
// host and on the device, over pcb_gumbel_tree.h (the quantities of a node, the root's scores, CHOOSE) and pcb_gumbel_leaves.h
// (the leaf loop, pending visits, repeats), both of which stay as they are: k_gumbel_tree_leaves (pcb_gumbel_tree_leaves.hip)
// composes the pieces below with child c of the current node in lane c of a group, and tools/gumbel_tree_leaves_check.cpp -- a
// CPU program -- composes them serially.  The other phases are the existing functions: pcb_gumbel.h:gumbel_begin,
// pcb_puct_leaves.h:leaves_absorb, pcb_gumbel_tree.h:tree_choose.  pcbenv/search.py:gumbel_search(node_rule="gumbel",
// leaves=L) is the specification.
//
// The rule of a node with pending visits.  pi' of a node is pcb_gumbel_tree.h's, from visits, value_sum and prior alone -- no
// virtual loss enters q or vmix, and max_b n_b inside sigma is the absorbed count -- so it is the same for every leaf of a
// launch.  A pending visit is counted as a visit and as nothing else:
//   m_c  = (int64) n_c + pn_c,  pn_c = pending(fc + c)
//   Msum = sum_c m_c                                        (64-bit integer: at most 64 terms below 2^32 in size)
//   t_c  = pi_c - (double) m_c / (1.0 + (double) Msum)
// and the search goes to the argmax of t_c, ties to the lowest c.  The node rule exists to make visit counts track pi'; with
// pi' frozen during a launch, the L descents through a node are distributed exactly as L sequential one-leaf visits with that
// pi' would be.  With pending == 0, t_c has the bits of pcb_gumbel_tree::excess.
//
// The order.  pending is data: Msum == -1 (damaged pending or visits only) makes the quotient infinite or NaN.  A NaN t_c
// counts as -inf: `ordered` below maps it there before any comparison, in the serial loop and in the lanes alike, so
// pcb_tree::beats sees numbers only and is a total order (larger t first, the lower c on equal t): the butterfly argmax and
// the loop agree whatever pending holds.
//
// The identities (tests/test_gumbel_tree_leaves_model.py, tests/test_gumbel_tree_leaves_gpu.py):
//   I1  with L == 1 and pending all zero every tensor pcbenv_gumbel_tree_advance writes gets the same bits; the differences
//       are pending itself and ABSORB taking it off again.  On trees with non-negative visits.
//   I2  after the ABSORB of every SELECT, pending is zero: pcbenv_puct_move(REROOT) and pcbenv_gumbel_tree_advance take the
//       tree as it is.
//   I3  BEGIN, ABSORB and CHOOSE have the bits of gumbel_begin, leaves_absorb and tree_choose on every case.
//
// What "bit for bit" covers.  children_ok checks a child range against N and C, not against the other ranges of the tree.  On a
// damaged tree whose ranges overlap -- a node among its own descendants, a range that takes in the root's children -- a descent
// can meet a slot twice.  Every store still stays inside the tensors, but the VALUES of pending are then not specified: the
// kernel carries the pending count of the node it stands at, and of the root's children, in registers, where the loop below
// reads memory again, so the two may differ.  Trees whose ranges are disjoint, healthy or damaged, are covered, as in
// pcb_gumbel_leaves.h, whose kernel does the same.
//
// The promise of pcb_puct.h holds here too: k and fc are compared with C and N before they address anything; sim_index
// addresses the table only while 0 <= t < n; pending, a table entry and a counter are data.
#pragma once
#include "pcb_gumbel_tree.h"
#include "pcb_gumbel_leaves.h"

namespace pcb_gumbel_tree_leaves {

using namespace pcb_gumbel_tree;
using pcb_puct_leaves::leaf_row;
using pcb_puct_leaves::MAX_LEAVES;
using pcb_puct_leaves::repeats;
using pcb_puct_leaves::undo_pending;
using pcb_puct_leaves::with_pending;
// pcb_gumbel.h and pcb_puct_leaves.h both have a wrapping increment of the same text; the one of pending is meant here
PCB_TREE_HD inline int pend_more(int n) { return pcb_puct_leaves::one_more(n); }

// a NaN counts as -inf
PCB_TREE_HD inline double ordered(double t) { return t == t ? t : pcb_tree::neg_inf(); }
// pcb_gumbel_tree.h:excess with the pending visits counted as visits; Msum = sum_c m_c
PCB_TREE_HD inline double excess(double pi, int visits_c, int pending_c, long long Msum) {
    return ordered(pi - (double)with_pending(visits_c, pending_c) / (1.0 + (double)Msum));
}

// the child the search goes to from `node`: the argmax of t_c, ties to the lowest child
PCB_TREE_HD inline int node_child(const Root &r, const Rule &q, const int *pending, int node, int k, int fc) {
    double lg[MAX_CHILDREN], sg[MAX_CHILDREN], pi[MAX_CHILDREN];
    node_logits(r, q, node, k, fc, lg, sg);
    for (int c = 0; c < k; c++) lg[c] = improved(lg[c], sg[c]);
    node_policy(lg, k, pi);
    long long Msum = 0;
    for (int c = 0; c < k; c++) Msum += with_pending(r.visits[fc + c], pending[fc + c]);  // at most 64 terms below 2^32: no overflow
    int best_c = -1;
    double best = 0.0;
    for (int c = 0; c < k; c++) {
        const double t = excess(pi[c], r.visits[fc + c], pending[fc + c], Msum);
        if (best_c < 0 || beats(t, c, best, best_c)) { best = t; best_c = c; }
    }
    return best_c;
}

// pcb_gumbel_leaves.h:descend_from with the node rule above in the place of the pending-visit PUCT score: from level d at
// `node` on; the levels above are the caller's.  Returns true if the descent was a repeat (nothing else is written then, and
// no pending visit stays).
PCB_TREE_HD inline bool tree_descend_from(const Root &r, const Rule &q, int *pending, int rows, int row, int node, int d, int *paths, int *path_len,
                                          int *selected, unsigned *err) {
    for (;; d++) {
        const int k = r.num_children[node], fc = r.first_child[node];
        if (d >= r.T || stops(r.terminal[node], k)) break;
        if (!children_ok(fc, k, r.N, r.C)) { *err |= ERR_TREE; break; }
        const int c = node_child(r, q, pending, node, k, fc);
        pending[node] = pend_more(pending[node]);
        node = fc + c;
        for (int i = 0; i < 3; i++) paths[step_major(d, rows, row, i)] = r.node_action[3 * node + i];
    }
    if (repeats(r.terminal[node], r.num_children[node], pending[node])) {
        *err |= undo_pending(r, pending, node, d);
        return true;
    }
    pending[node] = pend_more(pending[node]);
    selected[row] = node;
    path_len[row] = d;
    return false;
}

// pcb_gumbel_leaves.h:gumbel_leaves_select with three replacements: the root's scores are tree_root_scores', every level d >= 1
// is tree_descend_from's, and the one descent of a spent budget is tree_descend_from from the root.  considered [Mc + 1, n];
// sim_index: this root's element; sim_visits [C]: its row; pending [N]: its row; selected, path_len [P * L], paths [T, P * L,
// 3]: the whole tensors.  At most T levels per leaf.
PCB_TREE_HD inline unsigned tree_leaves_select(const Root &r, const Rule &q, int *pending, int L, const int *considered, int *sim_index, int *sim_visits,
                                               int *paths, int *path_len, int *selected) {
    unsigned err = 0u;
    const int rows = r.P * L, row0 = leaf_row(r.p, L, 0);
    const int k = r.num_children[0], fc = r.first_child[0];
    const bool halts = stops(r.terminal[0], k);
    int l = 0;
    if (halts || !children_ok(fc, k, r.N, r.C) || *sim_index < 0) {  // no descent: the root itself, once
        if (!halts) err |= ERR_TREE;
        pending[0] = pend_more(pending[0]);
        selected[row0] = 0;
        path_len[row0] = 0;
        l = 1;
    } else {
        double s[MAX_CHILDREN], x[MAX_CHILDREN];
        tree_root_scores(r, q, k, fc, s, x);  // once: no leaf changes what they read
        const long long table_row = (long long)considered_candidates(q.Mc, k) * q.n;
        for (; l < L; l++) {
            const int t = *sim_index, row = row0 + l;
            if (!scheduled(t, q.n)) {  // out of budget: one descent by the node rule from the root, and no more
                if (l > 0 || tree_descend_from(r, q, pending, rows, row, 0, 0, paths, path_len, selected, &err)) break;
                continue;
            }
            const int c = best_at(s, sim_visits, k, considered[table_row + t]);
            pending[0] = pend_more(pending[0]);
            for (int i = 0; i < 3; i++) paths[step_major(0, rows, row, i)] = r.node_action[3 * (fc + c) + i];
            if (tree_descend_from(r, q, pending, rows, row, fc + c, 1, paths, path_len, selected, &err)) break;
            sim_visits[c] = pcb_gumbel::one_more(sim_visits[c]);  // a repeat does not get here: it consumes no simulation
            *sim_index = t + 1;
        }
    }
    for (; l < L; l++) { selected[leaf_row(r.p, L, l)] = -1; path_len[leaf_row(r.p, L, l)] = -1; }
    return err;
}

}  // namespace pcb_gumbel_tree_leaves
