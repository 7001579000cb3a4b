// pcb_frontier.h -- the frontier step of pcbenv_frontier_advance, stated once: one depth of a beam search over partial
// placements, for ONE root.  Plain C++17 that compiles alone, on the host and on the device: k_frontier_advance
// (pcb_frontier.hip) composes the pieces below with the rows of a root spread over the lanes of a wavefront, and
// tools/frontier_check.cpp -- a CPU program that replays call sequences against pcbenv/search.py:frontier_advance, the
// specification -- composes them serially (frontier_init, frontier_advance).  One IEEE operation per written operator (the
// build passes -ffp-contract=off); the one logarithm is pcb_ieee_math.h's.
//
// A root holds F = W * K rows, row r = p * F + i its slot i.  A row is a partial placement named by its path:
//   paths [T, P * F, 3] step-major | path_len [P * F], -1 = no row | cum_logp [P * F] float64
// in two sets the caller swaps, `in` (read) and `out` (written).  The evaluation of the in rows is pcb_puct.h's:
//   value float64, leaf_terminal uint8, cand_count [P * F] | cand_actions [P * F, K, 3] | cand_prior float32 [P * F, K].
// ADVANCE, in four steps.  (1) A row is live if path_len_in is in [0, T]; a value outside [-1, T] is no row and reports
// ERR_ROW; of a row that is not live nothing else is read.  (2) Live rows with leaf_terminal != 0 are finished: in
// increasing i, with v = value and a NaN counted as -inf, a row for which best_len == -1 or v > best_value becomes the
// root's best (best_value = v, best_len = its length, best_path rows d < that length = its path).  A finished row is
// never expanded.  (3) Live, unfinished rows with path_len_in < T and k = clamp(cand_count, 0, K) > 0 are expandable, the
// others are dropped.  Their score is value if prior_weight == 0 and value + prior_weight * cum_logp_in otherwise, a NaN
// counted as -inf; the order is the score descending, as doubles, ties to the lower i; the first n = min(W, expandable)
// are kept, i_w the kept row of rank w.  (4) Child c < k of rank w goes to slot w * K + c: the parent's path and then
// cand_actions[parent, c], path_len + 1, cum_logp_in[parent] + log_prior(cand_prior[parent, c]), parent_row = i_w.  Every
// other slot gets path_len_out = parent_row = -1 and nothing else.  live = the child rows written.
//
// Nothing read back from memory addresses anything: lengths are compared with T before they bound a copy, counts are
// clamped to K, candidate actions are copied as data.
#pragma once
#include "pcb_ieee_math.h"
#include "pcb_tree.h"

namespace pcb_frontier {

using pcb_tree::neg_inf;
using pcb_tree::step_major;

enum { PHASE_INIT = 1, PHASE_ADVANCE = 2, MAX_WIDTH = 64, MAX_CANDIDATES = 64, MAX_ROWS = 1024 };
enum : unsigned { ERR_ROW = 2u };  // bit 1: a path_len_in outside [-1, T]

// The whole tensors of a call and its sizes: what the kernel takes as its argument block, too.
struct Frontier {
    int phases, P, W, K, T;
    double prior_weight;
    const int *paths_in, *path_len_in;
    const double *cum_logp_in;
    int *paths_out, *path_len_out;
    double *cum_logp_out;
    int *parent_row, *live;
    double *best_value;
    int *best_len, *best_path;
    const double *value;
    const uint8_t *leaf_terminal;
    const int *cand_count, *cand_actions;
    const float *cand_prior;
    unsigned *errors;
};

PCB_TREE_HD inline int rows_of(int W, int K) { return W * K; }
// ---- step 1 --------------------------------------------------------------------------------------------------------
PCB_TREE_HD inline bool is_live(int len, int T) { return len >= 0 && len <= T; }
PCB_TREE_HD inline bool is_damaged(int len, int T) { return len < -1 || len > T; }
// ---- steps 2 and 3 ---------------------------------------------------------------------------------------------------
PCB_TREE_HD inline double not_nan(double x) { return x != x ? neg_inf() : x; }
PCB_TREE_HD inline int kept_candidates(int cand_count, int K) { return cand_count < 0 ? 0 : cand_count > K ? K : cand_count; }
PCB_TREE_HD inline bool is_expandable(int len, int T, int k) { return len < T && k > 0; }
// cum_logp is not read into the score with prior_weight == 0: no 0 * inf
PCB_TREE_HD inline double score_of(double value, double prior_weight, const double *cum_logp) {
    if (prior_weight == 0.0) return not_nan(value);
    const double weighted = prior_weight * *cum_logp;
    return not_nan(value + weighted);
}
// row (sb, ib) goes before row (sa, ia): the score descending, ties to the lower slot (-0.0 ties with +0.0)
PCB_TREE_HD inline bool goes_before(double sb, int ib, double sa, int ia) { return sb > sa || (sb == sa && ib < ia); }
// a finished row with value v replaces the best so far
PCB_TREE_HD inline bool is_better(double v, double best_value, int best_len) { return best_len == -1 || v > best_value; }
// ---- step 4 --------------------------------------------------------------------------------------------------------
// ln of a prior that is a positive, finite, normal float32; -inf of any other (read through the bits: no denormal mode)
PCB_TREE_HD inline double log_prior(float prior) {
    uint32_t b;
    memcpy(&b, &prior, 4);
    const uint32_t e = (b >> 23) & 0xffu;
    return (b >> 31) == 0u && e >= 1u && e <= 254u ? pcb_ieee::ieee_ln((double)prior) : neg_inf();
}

// ---- init ----------------------------------------------------------------------------------------------------------
PCB_TREE_HD inline void init_row(const Frontier &f, long long row, int i) {
    f.path_len_out[row] = i == 0 ? 0 : -1;
    if (i == 0) f.cum_logp_out[row] = 0.0;
    f.parent_row[row] = -1;
}
PCB_TREE_HD inline void init_scalars(const Frontier &f, int p) { f.live[p] = 1; f.best_len[p] = -1; f.best_value[p] = neg_inf(); }
PCB_TREE_HD inline void frontier_init(const Frontier &f, int p) {
    const int F = rows_of(f.W, f.K);
    for (int i = 0; i < F; i++) init_row(f, (long long)p * F + i, i);
    init_scalars(f, p);
}

// ---- advance -------------------------------------------------------------------------------------------------------
// Child c of the in row `parent` into the out row `row`: everything of step 4 but the path rows.
PCB_TREE_HD inline void make_child(const Frontier &f, long long row, long long parent, int i_w, int len, int c) {
    f.path_len_out[row] = len + 1;
    f.cum_logp_out[row] = f.cum_logp_in[parent] + log_prior(f.cand_prior[parent * f.K + c]);
    f.parent_row[row] = i_w;
}
PCB_TREE_HD inline void no_child(const Frontier &f, long long row) { f.path_len_out[row] = -1; f.parent_row[row] = -1; }
// Element e of path row d of that child: the parent's below its length, the candidate at it.
PCB_TREE_HD inline int child_path(const Frontier &f, int rows, long long parent, int len, int c, int d, int e) {
    return d < len ? f.paths_in[step_major(d, rows, (int)parent, e)] : f.cand_actions[(parent * f.K + c) * 3 + e];
}

// One root, serially.  `taken` and `kept`: F and W ints of the caller's.  Returns the error bits.
PCB_TREE_HD inline unsigned frontier_advance(const Frontier &f, int p, unsigned char *taken, int *kept) {
    const int F = rows_of(f.W, f.K), rows = f.P * F;
    const long long row0 = (long long)p * F;
    unsigned err = 0u;
    // steps 1 and 2
    for (int i = 0; i < F; i++) {
        const long long r = row0 + i;
        const int len = f.path_len_in[r];
        taken[i] = 1;  // not expandable, until step 3 says otherwise
        if (is_damaged(len, f.T)) err |= ERR_ROW;
        if (!is_live(len, f.T)) continue;
        if (f.leaf_terminal[r] != 0) {
            const double v = not_nan(f.value[r]);
            if (is_better(v, f.best_value[p], f.best_len[p])) {
                f.best_value[p] = v;
                f.best_len[p] = len;
                for (int d = 0; d < len; d++)
                    for (int e = 0; e < 3; e++) f.best_path[step_major(d, f.P, p, e)] = f.paths_in[step_major(d, rows, (int)r, e)];
            }
            continue;
        }
        if (is_expandable(len, f.T, kept_candidates(f.cand_count[r], f.K))) taken[i] = 0;
    }
    // step 3: W rounds, each takes the row that goes before all others left
    int n = 0;
    for (; n < f.W; n++) {
        int best = -1;
        double best_s = 0.0;
        for (int i = 0; i < F; i++) {
            if (taken[i]) continue;
            const double s = score_of(f.value[row0 + i], f.prior_weight, &f.cum_logp_in[row0 + i]);
            if (best < 0 || goes_before(s, i, best_s, best)) { best = i; best_s = s; }
        }
        if (best < 0) break;
        taken[best] = 1;
        kept[n] = best;
    }
    // step 4
    int live = 0;
    for (int w = 0; w < f.W; w++) {
        const long long parent = w < n ? row0 + kept[w] : 0;
        const int len = w < n ? f.path_len_in[parent] : 0, k = w < n ? kept_candidates(f.cand_count[parent], f.K) : 0;
        for (int c = 0; c < f.K; c++) {
            const long long row = row0 + (long long)w * f.K + c;
            if (c >= k) { no_child(f, row); continue; }
            make_child(f, row, parent, kept[w], len, c);
            for (int d = 0; d <= len; d++)
                for (int e = 0; e < 3; e++) f.paths_out[step_major(d, rows, (int)row, e)] = child_path(f, rows, parent, len, c, d, e);
            live++;
        }
    }
    f.live[p] = live;
    return err;
}

}  // namespace pcb_frontier
