/* pcbenv_gumbel_tree_leaves.h -- the full Gumbel rule with several simulations per launch, beyond include/pcbenv.h:
 * pcbenv_gumbel_tree_advance_leaves, the tree step of pcbenv_gumbel_tree_advance (pcbenv_gumbel_tree.h: the paper's non-root
 * rule and v_mix) with L leaves per root and launch, as pcbenv_gumbel_advance_leaves (pcbenv_gumbel_leaves.h) takes them.  An
 * addition next to pcbenv.h, pcbenv_search.h, pcbenv_priors.h, pcbenv_move.h, pcbenv_train.h, pcbenv_leaves.h, pcbenv_noise.h,
 * pcbenv_gumbel.h, pcbenv_gumbel_leaves.h and pcbenv_gumbel_tree.h, which stay as they are: the ABI version is pcbenv.h's and
 * is unchanged, libpcbenv.so exports the entry point below as well, and pcbenv/_gumbel_tree_leaves_lib.py binds it.
 *
 * Streams.  As pcbenv_gumbel_advance_leaves: the call only enqueues one kernel on its request's stream.
 *
 * What it replaces: nothing in the reference, which has no search.  pcbenv/search.py:gumbel_search(node_rule="gumbel",
 * leaves=L) is the specification -- gumbel_node_scores and gumbel_select_node with pending= below the root -- which the kernel
 * matches bit for bit.
 */
#ifndef PCBENV_GUMBEL_TREE_LEAVES_H
#define PCBENV_GUMBEL_TREE_LEAVES_H

#include "pcbenv_gumbel_leaves.h"
#include "pcbenv_gumbel_tree.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One step of P search trees under the full Gumbel rule, L = num_leaves descents per root and launch, one kernel launch on
 * req->stream.  The request is pcbenv_gumbel_leaves_request, the struct of pcbenv_gumbel_advance_leaves, as it is: the same
 * tensors, dtypes and layouts, the same phases PCBENV_GUMBEL_BEGIN, _ABSORB, _SELECT, _CHOOSE run in that order, the same error
 * bits, and the same stream contract -- the caller owns every tensor, the handle supplies the device and pcbenv_last_error
 * only.  Enqueue only, no allocation, no synchronisation.  Not meant to be captured into a hipGraph.  c_puct is never read.
 * The rule of a node with pending visits.  At a node a that does not stop and whose child range is checked, with k children at
 * fc, ch = fc + c, n_c = visits(ch), pn_c = pending(ch): logit_c, Nsum, q_c, S, Wv, Qv, own, vhat, vmix, qhat_c, sigma_c, x_c
 * and pi_c are pcbenv_gumbel_tree.h's "quantities of a node" exactly.  They read visits, value_sum and prior and never pending
 * -- max_b n_b inside sigma is the absorbed count too -- so pi' of a node is the same for every leaf of a launch.  Then
 *   m_c  = (int64) n_c + pn_c
 *   Msum = sum_c m_c                                         (64-bit integer)
 *   t_c  = pi_c - (double) m_c / (1.0 + (double) Msum)
 * float64, one IEEE operation per written operator, left to right, and the search goes to the argmax of t_c, ties to the
 * lowest c.  A pending visit is counted as a visit and nothing else: no virtual loss enters q or vmix.  The rule makes the
 * visit counts of a node track pi'; with pi' frozen during a launch, the L descents through a node are distributed exactly as
 * L sequential one-leaf visits with that pi' would be: |m_c - M pi_c| keeps the bound of the one-leaf rule.  With pending == 0,
 * t_c has the bits of pcbenv_gumbel_tree.h's t_c.
 * The order.  pending is data: it addresses nothing.  Msum == -1, which only damaged pending or visits produce, makes the
 * quotient infinite or NaN; a NaN t_c counts as -inf, so the order is total: the larger t first, the lower c on equal t.
 * PCBENV_GUMBEL_BEGIN.  pcbenv_gumbel_advance's, bit for bit; it does not touch pending.
 * PCBENV_GUMBEL_ABSORB.  pcbenv_puct_advance_leaves' PCBENV_TREE_ABSORB, as in pcbenv_gumbel_advance_leaves, bit for bit.
 * PCBENV_GUMBEL_CHOOSE.  pcbenv_gumbel_tree_advance's, bit for bit; it does not read pending.
 * PCBENV_GUMBEL_SELECT.  pcbenv_gumbel_advance_leaves' with three replacements.
 *   1. The scores of the root's children are pcbenv_gumbel_tree_advance's (v_mix at the root): score_c = (g_c + logit_c) +
 *      sigma_c with sigma_c as above at node 0.  They are computed once per launch and read no pending visit.
 *   2. From the node the root level chose, every level d >= 1 is the rule above, with pcbenv_gumbel_advance_leaves'
 *      bookkeeping: pending += 1 on every node left and on the node reached, at most T levels in all, and a child range that
 *      fails the check ORs bit 1 into *errors_dev and ends the descent there.
 *   3. Out of budget, t >= n: leaf 0 is one descent from the root by the rule above, level 0 too, and the counters are
 *      untouched; leaves l >= 1 get selected = path_len = -1.
 * Repeats are pcbenv_gumbel_advance_leaves': a descent that ends at a node that is not terminal, has no children and has
 * pending > 0 takes its pending visits back, the root's included, consumes no simulation -- sim_index and sim_visits stay as
 * they were before this leaf -- and ends the selection of the root: -1 for this and all later leaves.  The repeat's own path
 * rows hold what it passed.  A root that is terminal or has k == 0, one whose child range fails the check, and one with
 * sim_index[p] < 0 takes no descent, as there: leaf 0 gets selected = 0, path_len = 0 and pending(0) += 1, every later leaf
 * -1, and the last two conditions OR bit 1 into *errors_dev.
 * Identities.
 *   I1  With num_leaves == 1 and pending all zero every tensor pcbenv_gumbel_tree_advance writes gets the same bits; the
 *       differences are pending itself and ABSORB taking it off again.  On trees with non-negative visits.
 *   I2  After the ABSORB of every SELECT, pending is zero: pcbenv_puct_move(PCBENV_MOVE_REROOT) and pcbenv_gumbel_tree_advance
 *       take the tree as it is.
 *   I3  BEGIN, ABSORB and CHOOSE have the bits named above on every tree.
 * A damaged tree whose child ranges overlap (the check of a range is against N and C, not against the other ranges) lets a
 * descent meet a slot twice: every store stays inside the tensors, the values left in pending are not specified.
 * Layouts: pcbenv_gumbel_leaves.h's.  errors_dev may be NULL.
 * PCBENV_EINVAL: pcbenv_gumbel_advance_leaves' checks, in its order, with its messages; num_roots == 0 is a no-op success. */
int pcbenv_gumbel_tree_advance_leaves(const pcbenv *env, const pcbenv_gumbel_leaves_request *req);

#ifdef __cplusplus
}
#endif
#endif /* PCBENV_GUMBEL_TREE_LEAVES_H */
