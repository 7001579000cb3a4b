// pcb_puct_move.h -- the move of pcbenv_puct_move (include/pcbenv_move.h), stated once: the choice of the move from the
// root's children and the compaction of the chosen child's subtree into a tree of its own, for ONE root.  Plain C++17
// over pcb_puct.h's Root that compiles alone, on the host and on the device: k_puct_move (pcb_puct_move.hip) composes the
// pieces below with the slots of a root spread over the lanes of a wavefront, and tools/puct_move_check.cpp -- a CPU
// program -- composes them serially (move_choose, move_reroot).  pcbenv/search.py:puct_choose and puct_reroot are the
// specification.  The choice has no floating-point operation; root_value is one IEEE division.
//
// Why the compaction can run in place, going up in slot order: children are made after their parent, so parent(s) < s;
// every kept slot is >= m, its new slot is its rank among the kept ones, hence <= s - m, and a store never lands on a
// slot that is still to be read.
//
// The promise of pcb_puct.h holds here too: every slot number or count read back from memory is compared before it
// addresses anything.  move_reroot validates the whole tree before its first store to it: all or nothing per root.
#pragma once
#include "pcb_puct.h"

namespace pcb_move {

using pcb_puct::children_ok;
using pcb_puct::init_scalars;
using pcb_puct::init_slot;
using pcb_puct::Root;
using pcb_tree::ERR_TREE;
using pcb_tree::MAX_CHILDREN;

enum { PHASE_CHOOSE = 1, PHASE_REROOT = 2, MODE_GREEDY = 0, MODE_PROPORTIONAL = 1 };

// ---- the draw hash of pcb_sampler.h, restated for host and device ----------------------------------------------------
PCB_TREE_HD inline uint64_t mix64(uint64_t z) {  // splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// hi32 of the 64 random bits of root genv's draw number `step` under `seed`
PCB_TREE_HD inline uint32_t draw_hi32(uint64_t seed, int genv, uint64_t step) {
    return (uint32_t)(mix64(mix64(seed ^ 0x9E3779B97F4A7C15ull * ((uint64_t)(int64_t)genv + 1)) + step) >> 32);
}
// where in [0, total) the draw falls: h * total >> 32, unsigned
PCB_TREE_HD inline long long draw_rank(uint32_t h, long long total) { return (long long)(((uint64_t)h * (uint64_t)total) >> 32); }

// ---- choose --------------------------------------------------------------------------------------------------------
// (visits b, child b) beats (visits a, child a): the first maximum wins
PCB_TREE_HD inline bool more_visits(int vb, int cb, int va, int ca) { return vb > va || (vb == va && cb < ca); }
// the proportional draw applies; otherwise the greedy choice stands
PCB_TREE_HD inline bool draws(int mode, long long total) { return mode == MODE_PROPORTIONAL && total > 0; }
PCB_TREE_HD inline double mean_value(double value_sum, int visits) { return value_sum / (double)visits; }

// child_visits [C], child_actions [C, 3], move_action [3]: this root's rows.  Every element is written.
PCB_TREE_HD inline unsigned move_choose(const Root &r, int mode, uint64_t seed, uint64_t step_index, int first_root, int *child_visits,
                                        int *child_actions, double *root_value, int *move_slot, int *move_action) {
    unsigned err = 0u;
    int k = r.num_children[0];
    const int fc = r.first_child[0];
    if (k != 0 && !children_ok(fc, k, r.N, r.C)) { err |= ERR_TREE; k = 0; }
    long long total = 0;
    int best_c = -1, best_v = 0;
    for (int c = 0; c < r.C; c++) {
        const bool mine = c < k;
        const int v = mine ? r.visits[fc + c] : 0;
        child_visits[c] = v;
        for (int i = 0; i < 3; i++) child_actions[3 * c + i] = mine ? r.node_action[3 * (fc + c) + i] : 0;
        if (!mine) continue;
        total += v;
        if (best_c < 0 || more_visits(v, c, best_v, best_c)) { best_v = v; best_c = c; }
    }
    if (k > 0 && draws(mode, total)) {
        const long long at = draw_rank(draw_hi32(seed, first_root + r.p, step_index), total);
        long long prefix = 0;
        for (int c = 0; c < k; c++) {
            prefix += child_visits[c];
            if (prefix > at) { best_c = c; break; }
        }
    }
    *root_value = mean_value(r.value_sum[0], r.visits[0]);
    *move_slot = k > 0 ? fc + best_c : -1;
    for (int i = 0; i < 3; i++) move_action[i] = k > 0 ? child_actions[3 * best_c + i] : 0;
    return err;
}

// ---- reroot --------------------------------------------------------------------------------------------------------
PCB_TREE_HD inline bool resets(int reset, int m) { return reset != 0 || m == -1; }
PCB_TREE_HD inline bool count_ok(int n, int N) { return n >= 1 && n <= N; }
PCB_TREE_HD inline bool move_ok(int m, int n) { return m >= 0 && m < n; }
PCB_TREE_HD inline bool parent_ok(int parent, int s) { return parent >= 0 && parent < s; }
// what is known of slot s without looking at its parent's verdict: slots below m are out, m is in
enum { OUT = 0, IN = 1, ASK_PARENT = 2 };
PCB_TREE_HD inline int kept_at_sight(int s, int m, int parent) { return s == m ? IN : (s < m || parent < m) ? OUT : parent == m ? IN : ASK_PARENT; }
// the children of a kept node, in the used part of the tree
PCB_TREE_HD inline bool kept_children_ok(int first_child, int k, int n, int C) { return k == 0 || children_ok(first_child, k, n, C); }
// ranks rise by one per kept slot: the k slots first .. last are all kept iff their ranks span k - 1
PCB_TREE_HD inline bool range_kept(int rank_first, int rank_last, int k) { return rank_first >= 0 && rank_last >= 0 && rank_last - rank_first == k - 1; }

// One node as it travels from its old slot to its new one.
struct Node {
    int parent, depth, visits, num_children, first_child, action[3];
    double prior, value_sum, value_max;
    uint8_t terminal;
};
PCB_TREE_HD inline Node load_node(const Root &r, int s) {
    return Node{r.parent[s], r.depth[s], r.visits[s], r.num_children[s], r.first_child[s], {r.node_action[3 * s], r.node_action[3 * s + 1], r.node_action[3 * s + 2]},
                r.prior[s], r.value_sum[s], r.value_max[s], r.terminal[s]};
}
PCB_TREE_HD inline void store_node(const Root &r, int s, const Node &x) {
    r.parent[s] = x.parent; r.depth[s] = x.depth; r.visits[s] = x.visits; r.num_children[s] = x.num_children; r.first_child[s] = x.first_child;
    r.node_action[3 * s] = x.action[0]; r.node_action[3 * s + 1] = x.action[1]; r.node_action[3 * s + 2] = x.action[2];
    r.prior[s] = x.prior; r.value_sum[s] = x.value_sum; r.value_max[s] = x.value_max; r.terminal[s] = x.terminal;
}
// the node in the new tree: links through remap, depth from the new root; the new root is a root
PCB_TREE_HD inline Node rerooted(Node x, bool new_root, int parent_rank, int first_child_rank, int depth_m) {
    x.parent = new_root ? -1 : parent_rank;
    x.first_child = x.num_children > 0 ? first_child_rank : -1;
    x.depth = (int)((unsigned)x.depth - (unsigned)depth_m);  // depths are not validated: the difference wraps, it never traps
    if (new_root) { x.action[0] = 0; x.action[1] = 0; x.action[2] = 0; x.prior = 0.0; }
    return x;
}
PCB_TREE_HD inline void fill_remap(int *remap, int N, int v) { for (int s = 0; s < N; s++) remap[s] = v; }

// remap [N]: this root's row.  m: move_slot[p]; reset: reset[p], 0 without the tensor.
PCB_TREE_HD inline unsigned move_reroot(const Root &r, int m, int reset, int *remap) {
    if (resets(reset, m)) {
        pcb_puct::puct_init(r);
        fill_remap(remap, r.N, -1);
        return 0u;
    }
    const int n = *r.num_nodes;
    if (!count_ok(n, r.N) || !move_ok(m, n)) { fill_remap(remap, r.N, -1); return ERR_TREE; }
    if (m == 0) {
        for (int s = 0; s < r.N; s++) remap[s] = s < n ? s : -1;
        return 0u;
    }
    // the ranks of the kept slots
    bool ok = true;
    int count = 0;
    for (int s = 0; s < r.N; s++) {
        int verdict = OUT;
        if (s < n) {
            const int up = s >= 1 ? r.parent[s] : -1;
            if (s >= 1 && !parent_ok(up, s)) { ok = false; break; }
            verdict = kept_at_sight(s, m, up);
            if (verdict == ASK_PARENT) verdict = remap[up] >= 0 ? IN : OUT;
        }
        remap[s] = verdict == IN ? count++ : -1;
    }
    // the child ranges of the kept nodes
    for (int s = m; ok && s < n; s++) {
        if (remap[s] < 0) continue;
        const int k = r.num_children[s], fc = r.first_child[s];
        ok = kept_children_ok(fc, k, n, r.C) && (k == 0 || range_kept(remap[fc], remap[fc + k - 1], k));
    }
    if (!ok) { fill_remap(remap, r.N, -1); return ERR_TREE; }
    // the move, going up: a node lands at or below its own slot
    const int depth_m = r.depth[m];
    for (int s = m; s < n; s++) {
        if (remap[s] < 0) continue;
        const Node x = load_node(r, s);
        store_node(r, remap[s], rerooted(x, s == m, s == m ? -1 : remap[x.parent], x.num_children > 0 ? remap[x.first_child] : -1, depth_m));
    }
    for (int s = count; s < n; s++) init_slot(r, s);
    *r.num_nodes = count;
    return 0u;
}

}  // namespace pcb_move
