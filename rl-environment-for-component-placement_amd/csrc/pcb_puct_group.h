// pcb_puct_group.h -- the two PUCT phases a lane group runs, stated once: the absorb of one evaluation and the descent by
// PUCT scores.  Part of libpcbenv.so (CDNA4 / gfx950 only), device code only: k_puct_advance (pcb_puct.hip) runs them as
// its ABSORB and SELECT, k_gumbel_advance (pcb_gumbel.hip) as its ABSORB and as the levels below its Gumbel root level.
// k_puct_leaves (pcb_puct_leaves.hip) keeps phases of its own: they carry `pending` and registers from leaf to leaf.
//
// The rule of one root is pcb_puct.h; the mapping (G lanes per root, lane c at child c of the current node, `base` the
// group's first lane in the wavefront) is pcb_group.h's.  `a` is a kernel's argument block: PuctArgs and GumbelArgs name
// selected, path_len, paths, value, leaf_terminal, cand_count, cand_actions, cand_prior, K and c_puct alike.  What a lane
// loads and stores:
//   descent  lane c of the group owns child first_child + c of the current node.  Per level two load round trips: the
//            node's terminal, num_children, first_child and visits together, then the children's visits, value_sum and
//            prior -- consecutive slots, so a group's loads are contiguous; k_tree_advance has to gather them.  The group
//            argmax (pcb_tree::beats: the lowest child on ties) is a shuffle butterfly; the winner's action is copied to
//            the path row by lanes 0..2 while the next level's loads are already under way.
//   absorb   lanes c < k write one child slot each; lane 0 writes the node's fields and the scalars and walks the backup
//            chain -- one round trip per level: a node's parent, visits, value_sum and value_max are loaded together.
// The absorb is a function template over the argument block.  The descent is a text macro, expanded where the two copies
// of the loop stood: as a function template, the whole loop or one level of it, it reaches the optimiser in another shape
// and moves bytes in all ten kernels (profiles/model_harness_refactor.txt; pcb_group.h's argmax is the precedent).
#pragma once
#include "pcb_group.h"
#include "pcb_puct.h"

namespace pcb_puct {

// puct_absorb, the new children over the lanes; returns the error bits (the same in every lane)
template <int G, class Args> __device__ inline unsigned absorb_phase(const Root &r, const Args &a, int lane, int base) {
    const int selected = a.selected[r.p], count = *r.num_nodes;
    if (!slot_ok(selected, r.N) || count < 1 || count > r.N) return ERR_TREE;
    unsigned err = 0u;
    const int node = selected, depth = r.depth[node], nch = r.num_children[node], term = r.terminal[node];
    const int leaf_terminal = a.leaf_terminal[r.p], cand_count = a.cand_count[r.p];
    const double value = a.value[r.p], lo = *r.lo, hi = *r.hi;
    if (leaf_terminal != 0) {
        if (lane == 0) r.terminal[node] = 1;
    } else if (expands(leaf_terminal, nch, term)) {
        const int k = kept_candidates(cand_count, a.K, r.C);
        if (k > 0 && count + k <= r.N) {
            const long long row = (long long)r.p * a.K;
            if (lane < k) make_child(r, node, count + lane, depth, a.cand_actions + 3 * (row + lane), a.cand_prior[row + lane]);
            if (lane == 0) link_children(r, node, count, k);
        } else if (k > 0) err |= ERR_FULL;
    }
    unsigned up = 0u;
    if (lane == 0) {
        *r.lo = value < lo ? value : lo;
        *r.hi = value > hi ? value : hi;
        up = back_up(r, node, value);
    }
    err |= __shfl(up, base);
    return err;
}

}  // namespace pcb_puct

// ---- puct_select's levels from level d at `node` on, child first_child + c of the current node in lane c ------------------
// r, a, lane, base as above; lo, hi the root's value range; node, d and err are the caller's variables: the descent leaves
// node and d where it ended and ORs its error bits into err.
#define PCB_PUCT_DESCEND(G, r, a, lane, base, lo, hi, node, d, err) \
    for (; d < r.T; d++) { \
        const int term = r.terminal[node], k = r.num_children[node], fc = r.first_child[node], vis = r.visits[node]; \
        if (pcb_puct::stops(term, k)) break; \
        if (!pcb_puct::children_ok(fc, k, r.N, r.C)) { err |= pcb_puct::ERR_TREE; break; } \
        const bool mine = lane < k; \
        const int ch = fc + (mine ? lane : 0); \
        double s = mine ? pcb_puct::puct_score(r.value_sum[ch], r.visits[ch], r.prior[ch], lo, hi, a.c_puct, vis) : pcb_puct::neg_inf(); \
        PCB_GROUP_ARGMAX(G, mine, lane, s, c, pcb_puct::beats) \
        node = fc + __shfl(c, base);  /* lane 0's verdict: one node per group whatever the scores were */ \
        if (lane < 3) a.paths[pcb_puct::step_major(d, r.P, r.p, lane)] = r.node_action[3 * node + lane]; \
    }
