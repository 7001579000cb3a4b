// pcb_frontier_sample.h -- the frontier step of pcbenv_frontier_sample (include/pcbenv_frontier_sample.h), stated once:
// one depth of a stochastic beam search over partial placements (Kool, van Hoof and Welling, ICML 2019), for ONE root.
// Plain C++17 that compiles alone, on the host and on the device, over pcb_frontier.h (the rows, the best finished row and
// the children), pcb_puct_noise.h (the uniform stream) and pcb_ieee_math.h (ln and exp): k_frontier_sample
// (pcb_frontier_sample.hip) composes the pieces below with the rows of a root spread over the lanes of a wavefront, and
// tools/frontier_sample_check.cpp -- a CPU program that replays call sequences against
// pcbenv/search.py:frontier_sample_advance, the specification -- composes them serially (sample_init, sample_advance).
// One IEEE operation per written operator (the build passes -ffp-contract=off).
//
// Beside pcb_frontier.h's rows a row has its perturbed log-probability G (gumbel [P * F] float64, a third member of the in
// and out sets), and a root has a sample set of W slots, slot p * W + j: set_len (-1 = free), set_gumbel, set_logp,
// set_value and set_path [T, P * W, 3] step-major.  ADVANCE: steps 1 and 2 are pcb_frontier.h's.  (3) The contenders are
// the set entries (set_len in [0, T]; outside [-1, T] is no entry and reports ERR_SET), id j, and the live rows that are
// finished or expandable, id W + i; the key is G with a NaN counted as -inf.  (4) The order is pcb_frontier.h:goes_before
// over (key, id); the first min(W, contenders) win.  A set entry that did not win is freed; the m-th finished winner goes
// into the m-th lowest slot that holds no surviving entry; the expandable winners are the kept parents i_w.  (5) The
// children as pcb_frontier.h's step 4, with G = truncated(G_S, phi_c + g_c, Z) of the parent's G_S, g_c the standard Gumbel
// of draw GUMBEL_DRAWS + i_w of child c and Z the largest phi_c + g_c over the children with finite phi_c.
//
// The promise of pcb_frontier.h holds: nothing read back from memory addresses anything.
#pragma once
#include "pcb_frontier.h"
#include "pcb_puct_noise.h"

namespace pcb_frontier_sample {

using namespace pcb_frontier;
using pcb_ieee::ieee_exp;
using pcb_ieee::ieee_ln;

enum : unsigned { ERR_SET = 4u };  // bit 2: a set_len outside [-1, T]
// Draw number GUMBEL_DRAWS + i of child c is the Gumbel of child c of the parent in slot i < MAX_ROWS: above every draw
// number of pcb_puct_noise.h (0 .. BOOST_DRAW = 96) and pcb_gumbel.h (GUMBEL_DRAW = 128).
enum { GUMBEL_DRAWS = 256 };
static_assert((int)GUMBEL_DRAWS > (int)pcb_noise::BOOST_DRAW && (int)GUMBEL_DRAWS > 128, "the draws of a frontier lie above the noise and the Gumbel root draws");

// pcb_frontier.h's tensors (prior_weight is not read) and what the sample adds
struct Sample {
    Frontier f;
    uint64_t seed, step_index;
    int first_root;
    const double *gumbel_in;
    double *gumbel_out;
    int *set_len;
    double *set_gumbel, *set_logp, *set_value;
    int *set_path;
};

// ---- the truncated Gumbel, stated once --------------------------------------------------------------------------------
PCB_TREE_HD inline bool is_finite(double x) { return x - x == 0.0; }
PCB_TREE_HD inline double gumbel_of(uint64_t base, int c, int i_w) { return -ieee_ln(-ieee_ln(pcb_noise::uniform(base, c, GUMBEL_DRAWS + i_w))); }
PCB_TREE_HD inline double larger(double a, double b) { return b > a ? b : a; }
// G of a child with finite phi_c: G_c = phi_c + g_c conditioned on the largest of its siblings', Z, being the parent's G_S.
// The arguments of exp are <= 0 (an infinite one gives 0), those of ln in [2^-53, 2].
PCB_TREE_HD inline double truncated(double G_S, double G_c, double Z) {
    if (!is_finite(G_S)) return G_S;
    const double a = G_c - Z;
    if (a == 0.0) return G_S;
    const double e = ieee_exp(a);
    const double d = 1.0 - e;
    if (d <= 0.0) return G_S;
    const double v = (G_S - G_c) + ieee_ln(d);
    const double top = v > 0.0 ? v : 0.0, mag = v < 0.0 ? -v : v;
    return (G_S - top) - ieee_ln(1.0 + ieee_exp(-mag));
}
PCB_TREE_HD inline double child_gumbel(double G_S, double phi_c, double G_c, double Z) { return is_finite(phi_c) ? truncated(G_S, G_c, Z) : neg_inf(); }

// ---- the set ----------------------------------------------------------------------------------------------------------
PCB_TREE_HD inline bool is_entry(int len, int T) { return is_live(len, T); }
// finished row r of the in set into slot s of the set, everything but the path rows
PCB_TREE_HD inline void enter_set(const Sample &q, long long s, long long r, int len, double key) {
    q.set_len[s] = len;
    q.set_gumbel[s] = key;
    q.set_logp[s] = q.f.cum_logp_in[r];
    q.set_value[s] = q.f.value[r];
}

// ---- init -------------------------------------------------------------------------------------------------------------
PCB_TREE_HD inline void init_gumbel(const Sample &q, long long row, int i) { if (i == 0) q.gumbel_out[row] = 0.0; }
PCB_TREE_HD inline void sample_init(const Sample &q, int p) {
    frontier_init(q.f, p);
    init_gumbel(q, (long long)p * rows_of(q.f.W, q.f.K), 0);
    for (int j = 0; j < q.f.W; j++) q.set_len[(long long)p * q.f.W + j] = -1;
}

// ---- advance ----------------------------------------------------------------------------------------------------------
enum : unsigned char { NO_CONTENDER = 0, FINISHED = 1, EXPANDABLE = 2, ENTRY = 3 };

// One root, serially.  `kind`: W + F bytes, `won`: W ints, `kept`: W ints of the caller's.  Returns the error bits.
PCB_TREE_HD inline unsigned sample_advance(const Sample &q, int p, unsigned char *kind, int *won, int *kept) {
    const Frontier &f = q.f;
    const int W = f.W, F = rows_of(f.W, f.K), rows = f.P * F, slots = f.P * W;
    const long long row0 = (long long)p * F, slot0 = (long long)p * W;
    unsigned err = 0u;
    // step 3, the set slots
    for (int j = 0; j < W; j++) {
        const int len = q.set_len[slot0 + j];
        if (is_damaged(len, f.T)) err |= ERR_SET;
        kind[j] = is_entry(len, f.T) ? ENTRY : NO_CONTENDER;
    }
    // steps 1, 2 and 3, the rows
    for (int i = 0; i < F; i++) {
        const long long r = row0 + i;
        const int len = f.path_len_in[r];
        kind[W + i] = NO_CONTENDER;
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
            kind[W + i] = FINISHED;
        } else if (is_expandable(len, f.T, kept_candidates(f.cand_count[r], f.K))) {
            kind[W + i] = EXPANDABLE;
        }
    }
    // step 4: W rounds, each takes the contender that goes before all others left
    int winners = 0;
    for (; winners < W; winners++) {
        int best = -1;
        double best_s = 0.0;
        for (int id = 0; id < W + F; id++) {
            if (kind[id] == NO_CONTENDER || (kind[id] & 0x80)) continue;
            const double s = not_nan(id < W ? q.set_gumbel[slot0 + id] : q.gumbel_in[row0 + id - W]);
            if (best < 0 || goes_before(s, id, best_s, best)) { best = id; best_s = s; }
        }
        if (best < 0) break;
        kind[best] |= 0x80;  // taken
        won[winners] = best;
    }
    for (int j = 0; j < W; j++)
        if (kind[j] == ENTRY) q.set_len[slot0 + j] = -1;  // an entry that did not win
    int n = 0, slot = 0;
    for (int m = 0; m < winners; m++) {
        const int id = won[m], what = kind[id] & 0x7f;
        if (what == EXPANDABLE) kept[n++] = id - W;
        if (what != FINISHED) continue;
        while (kind[slot] == (ENTRY | 0x80)) slot++;  // the lowest slot left that holds no surviving entry
        const long long r = row0 + id - W, s = slot0 + slot;
        const int len = f.path_len_in[r];
        enter_set(q, s, r, len, not_nan(q.gumbel_in[r]));
        for (int d = 0; d < len; d++)
            for (int e = 0; e < 3; e++) q.set_path[step_major(d, slots, (int)s, e)] = f.paths_in[step_major(d, rows, (int)r, e)];
        slot++;
    }
    // step 5
    const uint64_t base = pcb_noise::draw_base(q.seed, q.first_root + p, q.step_index);
    int live = 0;
    for (int w = 0; w < W; w++) {
        const long long parent = w < n ? row0 + kept[w] : 0;
        const int len = w < n ? f.path_len_in[parent] : 0, k = w < n ? kept_candidates(f.cand_count[parent], f.K) : 0;
        const double G_S = w < n ? not_nan(q.gumbel_in[parent]) : 0.0;
        double Z = neg_inf();
        for (int c = 0; c < f.K; c++) {
            const long long row = row0 + (long long)w * f.K + c;
            if (c >= k) { no_child(f, row); continue; }
            make_child(f, row, parent, kept[w], len, c);
            for (int d = 0; d <= len; d++)
                for (int e = 0; e < 3; e++) f.paths_out[step_major(d, rows, (int)row, e)] = child_path(f, rows, parent, len, c, d, e);
            const double phi = f.cum_logp_out[row];
            if (is_finite(phi)) Z = larger(Z, phi + gumbel_of(base, c, kept[w]));
            live++;
        }
        for (int c = 0; c < k; c++) {
            const long long row = row0 + (long long)w * f.K + c;
            const double phi = f.cum_logp_out[row];
            q.gumbel_out[row] = child_gumbel(G_S, phi, phi + gumbel_of(base, c, kept[w]), Z);
        }
    }
    f.live[p] = live;
    return err;
}

}  // namespace pcb_frontier_sample
