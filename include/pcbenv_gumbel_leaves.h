/* pcbenv_gumbel_leaves.h -- Gumbel root search with several simulations per launch, beyond include/pcbenv.h:
 * pcbenv_gumbel_advance_leaves, the tree step of pcbenv_gumbel_advance (pcbenv_gumbel.h) with L leaves per root and launch,
 * selected with the pending visits of pcbenv_puct_advance_leaves (pcbenv_leaves.h).  An addition next to pcbenv.h,
 * pcbenv_search.h, pcbenv_priors.h, pcbenv_move.h, pcbenv_train.h, pcbenv_leaves.h, pcbenv_noise.h and pcbenv_gumbel.h,
 * which stay as they are: the ABI version is pcbenv.h's and is unchanged, libpcbenv.so exports the entry point below as well,
 * and pcbenv/_gumbel_leaves_lib.py binds it.
 *
 * Streams.  As pcbenv_puct_advance: the call only enqueues one kernel on its request's stream.
 *
 * What it replaces: nothing in the reference, which has no search.  Sequential Halving sends the consecutive simulations of
 * a round to different root children, so the L descents of a launch start in different subtrees by construction; an
 * evaluator sees P * L nodes at once and one launch backs all of them up.  pcbenv/search.py:gumbel_search(leaves=L) is the
 * specification, which the kernel matches bit for bit.
 */
#ifndef PCBENV_GUMBEL_LEAVES_H
#define PCBENV_GUMBEL_LEAVES_H

#include "pcbenv_gumbel.h"
#include "pcbenv_leaves.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One step of P PUCT trees whose root level is a Gumbel search, L = num_leaves descents per root and launch: the tensors of
 * pcbenv_gumbel_request (same names, dtypes and layouts) and pending int32 [P, N] of pcbenv_puct_leaves_request, the exchange
 * tensors with the leaf extent of pcbenv_leaves.h: row r = p * L + l is leaf l of root p.  One kernel launch on req->stream.
 * The caller owns every tensor; the handle supplies the device and pcbenv_last_error only.  Enqueue only, no allocation, no
 * synchronisation.  Not meant to be captured into a hipGraph.  N, C, T, K, n, Mc as in pcbenv_gumbel.h.
 * phases is a set of PCBENV_GUMBEL_BEGIN, _ABSORB, _SELECT, _CHOOSE (pcbenv_gumbel.h: the same values); one launch runs them
 * in that order.  The search of a move is BEGIN | SELECT, then per evaluation ABSORB | SELECT (the last one ABSORB alone),
 * then CHOOSE.  A tree is initialised by pcbenv_puct_advance_leaves(PCBENV_TREE_INIT), which zeroes pending, and rerooted by
 * pcbenv_puct_move(PCBENV_MOVE_REROOT): pending is zero after the ABSORB of every SELECT.
 * PCBENV_GUMBEL_BEGIN, PCBENV_GUMBEL_CHOOSE.  pcbenv_gumbel_advance's, word for word and bit for bit.  BEGIN does not touch
 * pending and CHOOSE does not read it.
 * PCBENV_GUMBEL_ABSORB.  pcbenv_puct_advance_leaves' PCBENV_TREE_ABSORB, word for word: the leaves in order, a row with
 * selected == -1 skipped and none of its inputs read, the all-or-nothing expansion, the same error bits, pending -= 1 on
 * every node of each backup chain.
 * PCBENV_GUMBEL_SELECT.  The scores score_c = (g_c + logit_c) + sigma_c of the root's children are pcbenv_gumbel.h's
 * "quantities of a root".  They read visits and value_sum, never pending, and SELECT stores nothing to the tree but
 * pending: they are the same for every leaf of a launch.
 * A root that is terminal or has k == 0, one whose child range fails the check, and one with sim_index[p] < 0 takes no
 * descent: leaf 0 gets selected = 0, path_len = 0 and pending(0) += 1 (ABSORB's walk takes it off again), every later leaf
 * selected = path_len = -1, and no simulation is consumed.  The last two conditions OR bit 1 into *errors_dev.
 * Otherwise, for l = 0 .. L - 1 in that order, with t = sim_index[p] as the leaves before this one left it:
 *   scheduled, t < n.  v = considered[m * n + t], S = the children with sim_visits[p, c] == v, or all k if there is none,
 *     c* = the argmax of score_c over S, ties to the lowest c; pending(0) += 1, paths[0, r, :] = node_action(fc + c*), and
 *     from level 1 at node fc + c* the descent is pcbenv_puct_advance_leaves' SELECT exactly: its score with pending,
 *     pending += 1 on every node left and on the node reached, at most T levels in all.
 *   out of budget, t >= n.  Leaf 0 is one descent of pcbenv_puct_advance_leaves from the root, level 0 by its score too,
 *     and the counters are untouched: what pcbenv_gumbel_advance does.  At a leaf l >= 1 the selection of the root ends: this
 *     and all later leaves get selected = path_len = -1 and add no pending visit.
 *   a repeat (pcbenv_leaves.h: the descent ends at a node that is not terminal, has no children and has pending > 0) takes
 *     its pending visits back, the root's included, consumes no simulation -- sim_index and sim_visits stay as they were
 *     before this leaf -- and ends the selection of the root: -1 for this and all later leaves.  The child stays at count v,
 *     so the next leaf would choose it again.  The repeat's own path rows hold what it passed.
 *   otherwise selected[r], path_len[r] and the path rows are written, and sim_visits[p, c*] += 1, sim_index[p] = t + 1.
 * With num_leaves == 1 and pending all zero every tensor pcbenv_gumbel_advance writes gets the same bits; the differences
 * are pending itself and ABSORB taking it off again.
 * Layouts (int32 unless said): the tree, the budget and CHOOSE's outputs as in pcbenv_gumbel.h; pending [P, N]; selected,
 * path_len [P * L]; paths [T, P * L, 3]; value float64 [P * L]; leaf_terminal uint8 [P * L]; cand_count [P * L]; cand_actions
 * [P * L, K, 3]; cand_prior float32 [P * L, K].  errors_dev may be NULL.
 * PCBENV_EINVAL (checked before any device call, in this order): null request; struct_size not
 * sizeof(pcbenv_gumbel_leaves_request); phases 0 or with unknown bits, then CHOOSE together with SELECT; num_roots < 0;
 * capacity < 1; max_children outside [1, PCBENV_MAX_TREE_CHILDREN]; max_steps < 1; num_leaves outside
 * [1, PCBENV_MAX_PUCT_LEAVES]; num_roots * num_leaves above 2^31 - 1; num_candidates < 1 (ABSORB); num_simulations < 1;
 * max_considered outside [1, 64]; reserved or reserved2 != 0; c_visit or c_scale not finite or negative; a null tensor among
 * num_nodes ... reward_hi and pending (every phase); null sim_index or sim_visits (BEGIN, SELECT, CHOOSE); null selected
 * (ABSORB, SELECT); null path_len, paths or considered (SELECT); null value, leaf_terminal, cand_count, cand_actions or
 * cand_prior (ABSORB); null move_slot, move_action, child_weights, child_policy, child_actions or root_value (CHOOSE); a
 * float64 tensor not 8-byte aligned; cand_prior (ABSORB) or child_policy (CHOOSE) not 4-byte aligned; null handle.
 * num_roots == 0 is a no-op success. */
typedef struct pcbenv_gumbel_leaves_request {
    uint32_t struct_size; int32_t phases;            /* BEGIN, ABSORB, SELECT, CHOOSE in that order; SELECT|CHOOSE is EINVAL */
    int32_t num_roots /*P*/, capacity /*N node slots per root*/, max_children /*C*/, max_steps /*T*/, num_candidates /*K*/;
    int32_t num_simulations /*n*/, max_considered /*Mc*/, first_root /*global index of root 0 in the draw hash*/, reserved /*0*/;
    double c_puct, c_visit, c_scale;
    uint64_t seed, step_index;                       /* of the Gumbel draws */
    int32_t num_leaves /*L*/, reserved2 /*0*/;
    /* the tree, caller-owned device memory, root-major */
    int32_t *num_nodes;                              /* [P] */
    int32_t *parent, *depth, *visits, *num_children, *first_child; /* [P, N] */
    int32_t *node_action;                            /* [P, N, 3] */
    double *prior, *value_sum, *value_max;           /* [P, N] */
    uint8_t *terminal;                               /* [P, N] */
    double *reward_lo, *reward_hi;                   /* [P] */
    int32_t *pending;                                /* [P, N] visits selected and not yet absorbed */
    /* exchange with the evaluator (tuple format, step-major), row r = p * L + l */
    int32_t *selected, *path_len;                    /* [P * L]   written by SELECT; -1: no leaf */
    int32_t *paths;                                  /* [T, P * L, 3]: rows t < path_len[r] written, the others untouched */
    const double *value; const uint8_t *leaf_terminal; const int32_t *cand_count, *cand_actions; const float *cand_prior; /* read by ABSORB */
    /* the budget of the move */
    int32_t *sim_index;                              /* [P]: scheduled simulations made */
    int32_t *sim_visits;                             /* [P, C]: of them, per root child */
    const int32_t *considered;                       /* [Mc + 1, n] */
    /* written by CHOOSE */
    int32_t *move_slot;                              /* [P] */
    int32_t *move_action;                            /* [P, 3] */
    int32_t *child_weights;                          /* [P, C] */
    float *child_policy;                             /* [P, C] */
    int32_t *child_actions;                          /* [P, C, 3] */
    double *root_value;                              /* [P] */
    uint32_t *errors_dev;                            /* optional */
    void *stream;
} pcbenv_gumbel_leaves_request;
int pcbenv_gumbel_advance_leaves(const pcbenv *env, const pcbenv_gumbel_leaves_request *req);

#ifdef __cplusplus
}
#endif
#endif /* PCBENV_GUMBEL_LEAVES_H */
