// pcb_gumbel.h -- the root rule of pcbenv_gumbel_advance (include/pcbenv_gumbel.h), stated once: Gumbel-top-k candidates,
// Sequential Halving on g + logit + sigma(q) and the policy target softmax(logit + sigma(completed q)), for ONE root.  Plain
// C++17 that compiles alone, on the host and on the device, over pcb_puct.h (the tree, and every level below the root),
// pcb_puct_noise.h (the uniform stream) and pcb_ieee_math.h (ln and exp): k_gumbel_advance (pcb_gumbel.hip) composes the
// pieces below with child c of the root in lane c of a group, and tools/gumbel_check.cpp -- a CPU program -- composes them
// serially (gumbel_begin, gumbel_select, gumbel_choose; ABSORB is pcb_puct.h:puct_absorb itself).
// pcbenv/search.py:gumbel_scores, gumbel_select_root and gumbel_choose are the specification: the same operations in the
// same association, so the three agree bit for bit.  Every floating-point operation is + - * / or a comparison; the
// build passes -ffp-contract=off.
//
// The rule is stateless in its draws: g_c is draw number GUMBEL_DRAW of child c in the stream of (seed, global root, step
// index), so every launch of a move recomputes the same g.  What a move carries from launch to launch is sim_index, the
// scheduled simulations made, and sim_visits, how many of them each root child got: Sequential Halving's own counters,
// apart from the tree's visits, which a kept subtree brings along.
//
// The promise of pcb_puct.h holds here too: k and fc are compared with C and N before they address anything; sim_index
// addresses the table only when 0 <= t < n, and a table entry or a counter read back is only ever compared.
#pragma once
#include "pcb_puct_noise.h"

namespace pcb_gumbel {

using pcb_ieee::ieee_exp;
using pcb_ieee::ieee_ln;
using pcb_noise::draw_base;
using pcb_noise::uniform;
using pcb_puct::children_ok;
using pcb_puct::puct_score;
using pcb_puct::Root;
using pcb_puct::stops;
using pcb_tree::beats;
using pcb_tree::ERR_TREE;
using pcb_tree::MAX_CHILDREN;
using pcb_tree::step_major;

enum { PHASE_BEGIN = 1, PHASE_ABSORB = 2, PHASE_SELECT = 4, PHASE_CHOOSE = 8, GUMBEL_DRAW = 128, MAX_CONSIDERED = 64 };
constexpr double PRIOR_FLOOR = 0x1p-149;       // the smallest positive float32
constexpr double WEIGHT_ONE = 16777216.0;      // child_weights of a policy of 1: 2^24

// what a launch needs of the rule
struct Rule {
    double c_puct, c_visit, c_scale;
    uint64_t seed, step_index;
    int first_root, n /*num_simulations*/, Mc /*max_considered*/;
};

// ---- the quantities of a root child -------------------------------------------------------------------------------------
PCB_TREE_HD inline double gumbel(uint64_t base, int c) { return -ieee_ln(-ieee_ln(uniform(base, c, GUMBEL_DRAW))); }
// a zero, negative or NaN prior is at the floor
PCB_TREE_HD inline double logit(double prior) { return ieee_ln(prior > PRIOR_FLOOR ? (prior < 1.0 ? prior : 1.0) : PRIOR_FLOOR); }
PCB_TREE_HD inline double root_mean(double value_sum_0, int visits_0, double lo) { return visits_0 > 0 ? value_sum_0 / (double)visits_0 : lo; }
// pcb_puct.h:puct_score's q, completed with the root's mean value for a child without a visit
PCB_TREE_HD inline double completed_q(double value_sum_c, int visits_c, double vbar, double lo, double hi) {
    return hi > lo ? ((visits_c > 0 ? value_sum_c / (double)visits_c : vbar) - lo) / (hi - lo) : 0.0;
}
PCB_TREE_HD inline double sigma(double qhat, int most_visits, double c_visit, double c_scale) { return ((c_visit + (double)most_visits) * c_scale) * qhat; }
PCB_TREE_HD inline double improved(double logit_c, double sigma_c) { return logit_c + sigma_c; }
PCB_TREE_HD inline double score(double g, double logit_c, double sigma_c) { return (g + logit_c) + sigma_c; }
PCB_TREE_HD inline int larger(int a, int b) { return b > a ? b : a; }
PCB_TREE_HD inline double larger(double a, double b) { return b > a ? b : a; }
PCB_TREE_HD inline int considered_candidates(int Mc, int k) { return Mc < k ? Mc : k; }
// a counter one up; a counter the caller has damaged wraps, it never traps
PCB_TREE_HD inline int one_more(int v) { return (int)((unsigned)v + 1u); }
PCB_TREE_HD inline int weight(double pi) { return (int)(pi * WEIGHT_ONE + 0.5); }

// score [k] and improved logits x [k] of the children fc .. fc + k - 1 of the root (a range that children_ok has passed)
PCB_TREE_HD inline void root_scores(const Root &r, const Rule &q, int k, int fc, double *s, double *x) {
    const double lo = *r.lo, hi = *r.hi, vbar = root_mean(r.value_sum[0], r.visits[0], lo);
    int most = r.visits[fc];
    for (int c = 1; c < k; c++) most = larger(most, r.visits[fc + c]);
    const uint64_t base = draw_base(q.seed, q.first_root + r.p, q.step_index);
    for (int c = 0; c < k; c++) {
        const int ch = fc + c;
        const double lg = logit(r.prior[ch]), sg = sigma(completed_q(r.value_sum[ch], r.visits[ch], vbar, lo, hi), most, q.c_visit, q.c_scale);
        x[c] = improved(lg, sg);
        s[c] = score(gumbel(base, c), lg, sg);
    }
}
// the best score among the children whose counter is v -- among all k if there is none; ties to the lowest child
PCB_TREE_HD inline int best_at(const double *s, const int *sim_visits, int k, int v) {
    bool any = false;
    for (int c = 0; c < k; c++) any = any || sim_visits[c] == v;
    int best_c = -1;
    double best = 0.0;
    for (int c = 0; c < k; c++) {
        if (any && sim_visits[c] != v) continue;
        if (best_c < 0 || beats(s[c], c, best, best_c)) { best = s[c]; best_c = c; }
    }
    return best_c;
}

// ---- begin ---------------------------------------------------------------------------------------------------------
// sim_visits [C]: this root's row
PCB_TREE_HD inline void gumbel_begin(int C, int *sim_index, int *sim_visits) {
    *sim_index = 0;
    for (int c = 0; c < C; c++) sim_visits[c] = 0;
}

// ---- select --------------------------------------------------------------------------------------------------------
// pcb_puct.h:puct_select's loop from level *d at *node on
PCB_TREE_HD inline unsigned descend(const Root &r, double c_puct, int *paths, int *node_io, int *d_io) {
    unsigned err = 0u;
    const double lo = *r.lo, hi = *r.hi;
    int node = *node_io, d = *d_io;
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
    *node_io = node;
    *d_io = d;
    return err;
}
// the root is in its scheduled simulations: sim_index addresses the table
PCB_TREE_HD inline bool scheduled(int t, int n) { return t >= 0 && t < n; }
// considered [Mc + 1, n]; sim_index: this root's element; sim_visits [C]: its row.  Writes rows d < *path_len of paths
// [T, P, 3], *path_len, *selected, and for a scheduled simulation *sim_index and one element of sim_visits.
PCB_TREE_HD inline unsigned gumbel_select(const Root &r, const Rule &q, const int *considered, int *sim_index, int *sim_visits, int *paths,
                                          int *path_len, int *selected) {
    unsigned err = 0u;
    int node = 0, d = 0;
    const int k = r.num_children[0], fc = r.first_child[0];
    if (!stops(r.terminal[0], k)) {
        const int t = *sim_index;
        if (!children_ok(fc, k, r.N, r.C) || t < 0) err |= ERR_TREE;
        else {
            if (scheduled(t, q.n)) {
                double s[MAX_CHILDREN], x[MAX_CHILDREN];
                root_scores(r, q, k, fc, s, x);
                const int c = best_at(s, sim_visits, k, considered[(long long)considered_candidates(q.Mc, k) * q.n + t]);
                sim_visits[c] = one_more(sim_visits[c]);
                *sim_index = t + 1;
                node = fc + c;
                for (int i = 0; i < 3; i++) paths[step_major(0, r.P, r.p, i)] = r.node_action[3 * node + i];
                d = 1;
            }
            err |= descend(r, q.c_puct, paths, &node, &d);
        }
    }
    *selected = node;
    *path_len = d;
    return err;
}

// ---- choose --------------------------------------------------------------------------------------------------------
// sim_visits, child_weights, child_policy [C], child_actions [C, 3], move_action [3]: this root's rows.  Every element of
// the outputs is written.
PCB_TREE_HD inline unsigned gumbel_choose(const Root &r, const Rule &q, const int *sim_visits, int *move_slot, int *move_action, int *child_weights,
                                          float *child_policy, int *child_actions, double *root_value) {
    unsigned err = 0u;
    int k = r.num_children[0];
    const int fc = r.first_child[0];
    if (k != 0 && !children_ok(fc, k, r.N, r.C)) { err |= ERR_TREE; k = 0; }
    double s[MAX_CHILDREN], x[MAX_CHILDREN], e[MAX_CHILDREN];
    int best_c = -1;
    if (k > 0) {
        root_scores(r, q, k, fc, s, x);
        int most = sim_visits[0];
        double mx = x[0];
        for (int c = 1; c < k; c++) { most = larger(most, sim_visits[c]); mx = larger(mx, x[c]); }
        best_c = best_at(s, sim_visits, k, most);
        double Z = 0.0;
        for (int c = 0; c < k; c++) { e[c] = ieee_exp(x[c] - mx); Z = Z + e[c]; }  // in this order: it is the contract
        for (int c = 0; c < k; c++) e[c] = e[c] / Z;
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

// ---- the table -------------------------------------------------------------------------------------------------------
// row [n]: the considered visit count of every simulation for m candidates, 0 <= m
PCB_TREE_HD inline void considered_row(int m, int n, int *row) {
    if (m <= 1) {
        for (int t = 0; t < n; t++) row[t] = m == 1 ? t : 0;
        return;
    }
    int e = 0;
    while ((1 << e) < m) e++;
    int visits[MAX_CONSIDERED];
    for (int c = 0; c < m && c < MAX_CONSIDERED; c++) visits[c] = 0;
    int nc = m < MAX_CONSIDERED ? m : MAX_CONSIDERED, at = 0;
    while (at < n) {
        const int per = n / (e * nc), extra = per < 1 ? 1 : per;
        for (int x = 0; x < extra && at < n; x++)
            for (int c = 0; c < nc; c++) {
                if (at < n) row[at++] = visits[c];
                visits[c] = visits[c] + 1;
            }
        nc = nc / 2 < 2 ? 2 : nc / 2;
    }
}

}  // namespace pcb_gumbel
