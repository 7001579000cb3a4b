/* pcbenv_gumbel_tree.h -- the whole of "Policy improvement by planning with Gumbel" (Danihelka et al., ICLR 2022) on the
 * device, beyond include/pcbenv.h: pcbenv_gumbel_tree_advance, pcbenv_gumbel_advance (include/pcbenv_gumbel.h) with the
 * paper's second half -- its non-root rule at every level below the root, and v_mix, the prior-weighted completion of the
 * value of a child without a visit, at every node, the root included (section 5 and appendix D).  An addition next to
 * pcbenv.h, pcbenv_search.h, pcbenv_priors.h, pcbenv_move.h, pcbenv_train.h, pcbenv_leaves.h, pcbenv_noise.h, pcbenv_gumbel.h
 * and pcbenv_gumbel_leaves.h, which stay as they are: the ABI version is pcbenv.h's and is unchanged, libpcbenv.so exports
 * the entry point below as well, and pcbenv/_gumbel_tree_lib.py binds it.
 *
 * Streams.  As pcbenv_gumbel_advance: the call only enqueues one kernel on its request's stream.
 *
 * What it replaces: nothing in the reference, which has no search.  pcbenv/search.py:gumbel_node_scores,
 * gumbel_select_node, and gumbel_select_root and gumbel_choose with full=True are the specification, which the kernel matches
 * bit for bit.
 */
#ifndef PCBENV_GUMBEL_TREE_H
#define PCBENV_GUMBEL_TREE_H

#include "pcbenv_gumbel.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One step of P search trees under the full Gumbel rule, one kernel launch on req->stream.  The request is
 * pcbenv_gumbel_request, the struct of pcbenv_gumbel_advance: the same tensors, dtypes and layouts, the same phases
 * PCBENV_GUMBEL_BEGIN, _ABSORB, _SELECT, _CHOOSE run in that order, the same error bits, and the same stream contract --
 * the caller owns every tensor, the handle supplies the device and pcbenv_last_error only, nothing the library owns is read
 * or written and no bound buffers are needed.  Enqueue only, no allocation, no synchronisation, one kernel on req->stream.
 * Not meant to be captured into a hipGraph.  c_puct is never read: the rule has no exploration constant.
 * Quantities of a node a that does not stop (it is not terminal and has children) and whose child range is checked (1 <= k
 * <= C, 1 <= fc <= N - k, k = num_children(a), fc = first_child(a)) before it addresses anything; ch = fc + c, n_c =
 * visits(ch), lo = reward_lo[p], hi = reward_hi[p], the ROOT's value range at every node:
 *   pr_c    = prior(ch) > 2^-149 ? (prior(ch) < 1 ? prior(ch) : 1) : 2^-149;  logit_c = ln(pr_c)
 *   Nsum    = sum_c n_c                                  (64-bit integer)
 *   q_c     = value_sum(ch) / n_c                        (only where n_c > 0)
 *   S       = sum_c value_sum(ch)                        all k children
 *   Wv      = sum_{c: n_c > 0} pr_c ;  Qv = sum_{c: n_c > 0} pr_c * q_c
 *   own     = visits(a) - Nsum                           (64-bit)
 *   vhat    = own > 0 ? (value_sum(a) - S) / (double)own : (visits(a) > 0 ? value_sum(a) / visits(a) : lo)
 *   vmix    = (Nsum > 0 && Wv > 0.0) ? (vhat + ((double)Nsum / Wv) * Qv) / (1.0 + (double)Nsum) : vhat
 *   qhat_c  = hi > lo ? ((n_c > 0 ? q_c : vmix) - lo) / (hi - lo) : 0.0
 *   sigma_c = ((c_visit + (double)max_b n_b) * c_scale) * qhat_c
 *   x_c     = logit_c + sigma_c ; mx = max x ; e_c = exp(x_c - mx) ; Z = e_0 + ... + e_(k-1) ; pi_c = e_c / Z
 *   t_c     = pi_c - (double)n_c / (1.0 + (double)Nsum)
 * All of it float64, one IEEE operation per written operator, evaluated left to right; ln and exp are the library's own
 * (csrc/pcb_ieee_math.h).  Every sum over children is formed in child order from 0.0: the bits of a root depend neither on
 * C nor on the other roots of the batch.
 * vhat is the node's own evaluation recovered from the tree: a backup adds one value to a node and to every ancestor, so
 * value_sum(a) - S is the sum of the evaluations that ended at a and own is their count -- 1 for a node expanded at its first
 * visit, more for a leaf absorbed repeatedly, 0 or negative only in a hand-made or damaged tree, which is data, not an error.
 * No tensor is added to the tree: pcbenv_puct_move(PCBENV_MOVE_REROOT) keeps everything the rule reads.
 * Two deliberate departures from the paper: q is normalised by the search's [reward_lo, reward_hi], as everywhere in this
 * library, not per node; vhat is derived as above rather than stored.
 * PCBENV_GUMBEL_BEGIN, PCBENV_GUMBEL_ABSORB.  pcbenv_gumbel_advance's, word for word.
 * PCBENV_GUMBEL_SELECT.  pcbenv_gumbel_advance's with two changes.  In a scheduled simulation (0 <= t < n, t =
 * sim_index[p]) score_c = (g_c + logit_c) + sigma_c with sigma_c as above at node 0 -- g_c, the table, S, the ties and the
 * counter stores are unchanged.  Level 0 with t >= n and every level d >= 1 go to the argmax of t_c over the node's children,
 * ties to the lowest c; the path row is copied as before, at most T levels in all, and a child range that fails the check
 * ORs bit 1 into *errors_dev and ends the descent there.  SELECT never stores to the tree.
 * PCBENV_GUMBEL_CHOOSE.  pcbenv_gumbel_advance's with x_c and score_c as above at node 0.
 * Two identities.  With c_scale == 0, level 0 of every scheduled SELECT and every output of CHOOSE have
 * pcbenv_gumbel_advance's bits; for any c_scale the same holds at a root whose k children all have n_c > 0, where vmix is
 * not read.
 * PCBENV_EINVAL: pcbenv_gumbel_advance's checks, in its order, with its messages; num_roots == 0 is a no-op success. */
int pcbenv_gumbel_tree_advance(const pcbenv *env, const pcbenv_gumbel_request *req);

#ifdef __cplusplus
}
#endif
#endif /* PCBENV_GUMBEL_TREE_H */
