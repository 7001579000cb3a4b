// pcb_gumbel_tree.h -- the node rule of pcbenv_gumbel_tree_advance (include/pcbenv_gumbel_tree.h), stated once: the
// second half of "Policy improvement by planning with Gumbel" (Danihelka et al., ICLR 2022, section 5 and appendix D), for
// ONE node of ONE root.  At a node the search goes to argmax_c (pi'(c) - N(c) / (1 + sum_b N(b))), pi' = softmax(logit +
// sigma(completed q)), and the completed q of a child without a visit is v_mix, the node's value under its prior.  Plain
// C++17 that compiles alone, on the host and on the device, over pcb_gumbel.h (the root rule, whose draws, table and
// counters stay what they are): k_gumbel_tree (pcb_gumbel_tree.hip) composes the pieces below with child c of the current
// node in lane c of a group, and tools/gumbel_tree_check.cpp -- a CPU program -- composes them serially (gumbel_begin,
// tree_select, tree_choose; ABSORB is pcb_puct.h:puct_absorb itself).  pcbenv/search.py:gumbel_node_scores and
// gumbel_select_node are the specification: the same operations in the same association, so the three agree bit for bit.
// Every floating-point operation is + - * / or a comparison; the build passes -ffp-contract=off.
//
// The quantities of a node a that does not stop (pcb_puct::stops) and whose child range passed children_ok, k =
// num_children(a), fc = first_child(a), ch = fc + c, n_c = visits(ch), lo and hi the root's value range:
//   pr_c    = the clamped prior of pcb_gumbel::logit (floor 2^-149, cap 1);  logit_c = ln(pr_c)
//   Nsum    = sum_c n_c                                  (64-bit integer)
//   q_c     = value_sum(ch) / n_c                        (only where n_c > 0)
//   S       = sum_c value_sum(ch)                        all k children
//   Wv      = sum_{c: n_c > 0} pr_c ;  Qv = sum_{c: n_c > 0} pr_c * q_c
//   own     = visits(a) - Nsum                           (64-bit)
//   vhat    = own > 0 ? (value_sum(a) - S) / (double)own : (visits(a) > 0 ? value_sum(a) / visits(a) : lo)
//   vmix    = (Nsum > 0 && Wv > 0.0) ? (vhat + ((double)Nsum / Wv) * Qv) / (1.0 + (double)Nsum) : vhat
//   qhat_c  = hi > lo ? ((n_c > 0 ? q_c : vmix) - lo) / (hi - lo) : 0.0
//   sigma_c = pcb_gumbel::sigma(qhat_c, max_b n_b, c_visit, c_scale)
//   x_c     = logit_c + sigma_c ; mx = max x ; e_c = exp(x_c - mx) ; Z = e_0 + ... + e_(k-1) ; pi_c = e_c / Z
//   t_c     = pi_c - (double)n_c / (1.0 + (double)Nsum)
// Every sum over children is formed in child order from 0.0, as pcb_gumbel.h:gumbel_choose forms Z: the bits of a root do
// not depend on C, on the group width or on the batch.
//
// vhat is the node's own evaluation, recovered from the tree: back_up adds one value to a node and to every ancestor, so
// value_sum(a) - S is the sum of the evaluations that ended AT a and `own` is their count -- 1 for a node expanded at its
// first visit, more for a leaf absorbed repeatedly (after ERR_FULL, say), 0 or negative only in a hand-made or damaged tree,
// which is data, not an error.  No tensor is added to the tree, so pcbenv_puct_move(REROOT) keeps all the rule reads.
//
// Two deliberate departures from the paper: q is normalised by the search's [reward_lo, reward_hi], as everywhere in this
// library, not per node; and vhat is derived as above rather than stored.
//
// The promise of pcb_puct.h holds here too: k and fc are compared with C and N before they address anything.
#pragma once
#include "pcb_gumbel.h"

namespace pcb_gumbel_tree {

using namespace pcb_gumbel;

// ---- the quantities of a node ---------------------------------------------------------------------------------------------
PCB_TREE_HD inline double clamped_prior(double prior) { return prior > PRIOR_FLOOR ? (prior < 1.0 ? prior : 1.0) : PRIOR_FLOOR; }
// the node's own evaluation: S the sum of its children's value_sum, Nsum of their visits
PCB_TREE_HD inline double own_value(double value_sum_a, int visits_a, double S, long long Nsum, double lo) {
    const long long own = (long long)visits_a - Nsum;
    return own > 0 ? (value_sum_a - S) / (double)own : (visits_a > 0 ? value_sum_a / (double)visits_a : lo);
}
PCB_TREE_HD inline double mixed_value(double vhat, long long Nsum, double Wv, double Qv) {
    return (Nsum > 0 && Wv > 0.0) ? (vhat + ((double)Nsum / Wv) * Qv) / (1.0 + (double)Nsum) : vhat;
}
// pcb_gumbel.h:completed_q with the mean already formed: q_c of a visited child, vmix of any other
PCB_TREE_HD inline double completed(double q_or_vmix, double lo, double hi) { return hi > lo ? (q_or_vmix - lo) / (hi - lo) : 0.0; }
PCB_TREE_HD inline double excess(double pi, int visits_c, long long Nsum) { return pi - (double)visits_c / (1.0 + (double)Nsum); }

// logit [k] and sigma [k] of the children fc .. fc + k - 1 of `node` (a range that children_ok has passed); -> Nsum
PCB_TREE_HD inline long long node_logits(const Root &r, const Rule &q, int node, int k, int fc, double *lg, double *sg) {
    const double lo = *r.lo, hi = *r.hi;
    long long Nsum = 0;
    int most = r.visits[fc];
    double S = 0.0, Wv = 0.0, Qv = 0.0;
    for (int c = 0; c < k; c++) {  // in this order: it is the contract
        const int ch = fc + c, n_c = r.visits[ch];
        Nsum += (long long)n_c;
        most = larger(most, n_c);
        S = S + r.value_sum[ch];
        if (n_c > 0) {
            const double pr = clamped_prior(r.prior[ch]);
            Wv = Wv + pr;
            Qv = Qv + pr * (r.value_sum[ch] / (double)n_c);
        }
    }
    const double vmix = mixed_value(own_value(r.value_sum[node], r.visits[node], S, Nsum, lo), Nsum, Wv, Qv);
    for (int c = 0; c < k; c++) {
        const int ch = fc + c, n_c = r.visits[ch];
        lg[c] = logit(r.prior[ch]);
        sg[c] = sigma(completed(n_c > 0 ? r.value_sum[ch] / (double)n_c : vmix, lo, hi), most, q.c_visit, q.c_scale);
    }
    return Nsum;
}
// pi [k] = softmax(x) as gumbel_choose forms it
PCB_TREE_HD inline void node_policy(const double *x, int k, double *pi) {
    double mx = x[0];
    for (int c = 1; c < k; c++) mx = larger(mx, x[c]);
    double Z = 0.0;
    for (int c = 0; c < k; c++) { pi[c] = ieee_exp(x[c] - mx); Z = Z + pi[c]; }  // in this order: it is the contract
    for (int c = 0; c < k; c++) pi[c] = pi[c] / Z;
}
// the child the search goes to from `node`: the argmax of t_c, ties to the lowest child
PCB_TREE_HD inline int node_child(const Root &r, const Rule &q, int node, int k, int fc) {
    double lg[MAX_CHILDREN], sg[MAX_CHILDREN], pi[MAX_CHILDREN];
    const long long Nsum = node_logits(r, q, node, k, fc, lg, sg);
    for (int c = 0; c < k; c++) lg[c] = improved(lg[c], sg[c]);
    node_policy(lg, k, pi);
    int best_c = -1;
    double best = 0.0;
    for (int c = 0; c < k; c++) {
        const double t = excess(pi[c], r.visits[fc + c], Nsum);
        if (best_c < 0 || beats(t, c, best, best_c)) { best = t; best_c = c; }
    }
    return best_c;
}
// pcb_gumbel.h:root_scores with the completion above: score [k] and improved logits x [k] of the root's children
PCB_TREE_HD inline void tree_root_scores(const Root &r, const Rule &q, int k, int fc, double *s, double *x) {
    double lg[MAX_CHILDREN], sg[MAX_CHILDREN];
    node_logits(r, q, 0, k, fc, lg, sg);
    const uint64_t base = draw_base(q.seed, q.first_root + r.p, q.step_index);
    for (int c = 0; c < k; c++) {
        x[c] = improved(lg[c], sg[c]);
        s[c] = score(gumbel(base, c), lg[c], sg[c]);
    }
}

// ---- select --------------------------------------------------------------------------------------------------------
// pcb_gumbel.h:descend with the node rule in the place of PUCT's, from level *d at *node on
PCB_TREE_HD inline unsigned tree_descend(const Root &r, const Rule &q, int *paths, int *node_io, int *d_io) {
    unsigned err = 0u;
    int node = *node_io, d = *d_io;
    for (; d < r.T; d++) {
        const int k = r.num_children[node], fc = r.first_child[node];
        if (stops(r.terminal[node], k)) break;
        if (!children_ok(fc, k, r.N, r.C)) { err |= ERR_TREE; break; }
        node = fc + node_child(r, q, node, k, fc);
        for (int i = 0; i < 3; i++) paths[step_major(d, r.P, r.p, i)] = r.node_action[3 * node + i];
    }
    *node_io = node;
    *d_io = d;
    return err;
}
// pcb_gumbel.h:gumbel_select: the same table, S, ties and counter stores; the scores are tree_root_scores', the levels
// below -- and level 0 once the budget is spent -- tree_descend's
PCB_TREE_HD inline unsigned tree_select(const Root &r, const Rule &q, const int *considered, int *sim_index, int *sim_visits, int *paths, int *path_len,
                                        int *selected) {
    unsigned err = 0u;
    int node = 0, d = 0;
    const int k = r.num_children[0], fc = r.first_child[0];
    if (!stops(r.terminal[0], k)) {
        const int t = *sim_index;
        if (!children_ok(fc, k, r.N, r.C) || t < 0) err |= ERR_TREE;
        else {
            if (scheduled(t, q.n)) {
                double s[MAX_CHILDREN], x[MAX_CHILDREN];
                tree_root_scores(r, q, k, fc, s, x);
                const int c = best_at(s, sim_visits, k, considered[(long long)considered_candidates(q.Mc, k) * q.n + t]);
                sim_visits[c] = one_more(sim_visits[c]);
                *sim_index = t + 1;
                node = fc + c;
                for (int i = 0; i < 3; i++) paths[step_major(0, r.P, r.p, i)] = r.node_action[3 * node + i];
                d = 1;
            }
            err |= tree_descend(r, q, paths, &node, &d);
        }
    }
    *selected = node;
    *path_len = d;
    return err;
}

// ---- choose --------------------------------------------------------------------------------------------------------
// pcb_gumbel.h:gumbel_choose with tree_root_scores: the same outputs, every element written
PCB_TREE_HD inline unsigned tree_choose(const Root &r, const Rule &q, const int *sim_visits, int *move_slot, int *move_action, int *child_weights,
                                        float *child_policy, int *child_actions, double *root_value) {
    unsigned err = 0u;
    int k = r.num_children[0];
    const int fc = r.first_child[0];
    if (k != 0 && !children_ok(fc, k, r.N, r.C)) { err |= ERR_TREE; k = 0; }
    double s[MAX_CHILDREN], x[MAX_CHILDREN], e[MAX_CHILDREN];
    int best_c = -1;
    if (k > 0) {
        tree_root_scores(r, q, k, fc, s, x);
        int most = sim_visits[0];
        for (int c = 1; c < k; c++) most = larger(most, sim_visits[c]);
        best_c = best_at(s, sim_visits, k, most);
        node_policy(x, k, e);
    }
    for (int c = 0; c < r.C; c++) {
        const bool mine = c < k;
        child_weights[c] = mine ? weight(e[c]) : 0;
        child_policy[c] = mine ? (float)e[c] : 0.0f;
        for (int i = 0; i < 3; i++) child_actions[3 * c + i] = mine ? r.node_action[3 * (fc + c) + i] : 0;
    }
    *root_value = pcb_move::mean_value(r.value_sum[0], r.visits[0]);
    *move_slot = k > 0 ? fc + best_c : -1;
    for (int i = 0; i < 3; i++) move_action[i] = k > 0 ? child_actions[3 * best_c + i] : 0;
    return err;
}

}  // namespace pcb_gumbel_tree
