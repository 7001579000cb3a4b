/* pcbenv_gumbel.h -- Gumbel root search with sequential halving on the device, beyond include/pcbenv.h:
 * pcbenv_gumbel_advance, the tree step of a batched search whose ROOT level follows "Policy improvement by planning with
 * Gumbel" (Danihelka et al., ICLR 2022): the candidates are sampled without replacement by Gumbel-top-k, the simulation
 * budget is spent by Sequential Halving on g + logit + sigma(q), and the policy target is softmax(logit + sigma(completed
 * q)) instead of visit counts.  An addition next to pcbenv.h, pcbenv_search.h, pcbenv_priors.h, pcbenv_move.h,
 * pcbenv_train.h, pcbenv_leaves.h and pcbenv_noise.h, which stay as they are: the ABI version is pcbenv.h's and is
 * unchanged, libpcbenv.so exports the entry point below as well, and pcbenv/_gumbel_lib.py binds it.
 *
 * Streams.  As pcbenv_puct_advance: the call only enqueues one kernel on its request's stream.
 *
 * What it replaces: nothing in the reference, which has no search.  Below the root the search is pcbenv_puct_advance's;
 * at the root it is the rule above, where the priors live: in the tree, on the device.  pcbenv/search.py:gumbel_scores,
 * gumbel_select_root and gumbel_choose are the specification, which the kernel matches bit for bit.  The paper's non-root
 * rule and its v_mix completion are not part of it.
 */
#ifndef PCBENV_GUMBEL_H
#define PCBENV_GUMBEL_H

#include "pcbenv_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCBENV_GUMBEL_BEGIN 1
#define PCBENV_GUMBEL_ABSORB 2
#define PCBENV_GUMBEL_SELECT 4
#define PCBENV_GUMBEL_CHOOSE 8

/* One step of P PUCT trees whose root level is a Gumbel search (the tree tensors and the evaluator-exchange tensors of
 * pcbenv_puct_request, same names, dtypes and layouts), one kernel launch on req->stream.  The caller owns every tensor;
 * the handle supplies the device and pcbenv_last_error only: nothing the library owns is read or written and no bound
 * buffers are needed.  Enqueue only, no allocation, no synchronisation, one kernel on req->stream.  Not meant to be
 * captured into a hipGraph.  N = capacity node slots per root, C = max_children, T = max_steps, K = num_candidates,
 * n = num_simulations, Mc = max_considered.
 * phases is a set of PCBENV_GUMBEL_BEGIN, _ABSORB, _SELECT, _CHOOSE; one launch runs them in that order.  The search of a
 * move is BEGIN | SELECT, then per evaluation ABSORB | SELECT (the last one ABSORB alone), then CHOOSE.  A tree is
 * initialised by pcbenv_puct_advance(PCBENV_TREE_INIT) and rerooted by pcbenv_puct_move(PCBENV_MOVE_REROOT), which reads
 * move_slot as CHOOSE writes it.
 * Quantities of a root.  Let k = num_children(0) and fc = first_child(0); both are checked (1 <= k <= C, 1 <= fc <= N - k)
 * before they address anything.  m = min(Mc, k).  For every child c < k, with ch = fc + c and n_c = visits(ch):
 *   draw    base = mix64(mix64(seed ^ 0x9E3779B97F4A7C15 * (first_root + p + 1)) + step_index), pcbenv_noise.h's; draw
 *           number 128 of child c is w = mix64(base + 0x9E3779B97F4A7C15 * (64 * 128 + c + 1)), u = ((w >> 12) + 0.5) *
 *           2^-52, and g_c = -ln(-ln u).  The noise draws of pcbenv_noise.h use the numbers 0 .. 96: no key is shared.  A
 *           value depends on (seed, first_root + p, step_index, c) alone: never on P, on C or on the other children.
 *   logit   logit_c = ln(pr), pr = prior(ch) > 2^-149 ? (prior(ch) < 1 ? prior(ch) : 1) : 2^-149: a zero, negative or NaN
 *           prior is at the floor.
 *   value   range = reward_hi > reward_lo; vbar = visits(0) > 0 ? value_sum(0) / visits(0) : reward_lo;
 *           qhat_c = range ? ((n_c > 0 ? value_sum(ch) / n_c : vbar) - reward_lo) / (reward_hi - reward_lo) : 0 -- the
 *           min-max normalisation of pcbenv_puct_advance's q, completed with the root's mean value for a child without a
 *           visit.
 *   score   sigma_c = ((c_visit + (double)max_b n_b) * c_scale) * qhat_c, the maximum over the k children;
 *           score_c = (g_c + logit_c) + sigma_c.
 * All of it float64, one IEEE operation per written operator, evaluated left to right; ln and exp are the library's own,
 * written in IEEE + - * / alone (csrc/pcb_ieee_math.h), inside their stated domains: u and -ln u are positive normal
 * numbers, pr >= 2^-149, and exp only sees arguments <= 0.  The same bits everywhere.
 * PCBENV_GUMBEL_BEGIN.  sim_index[p] = 0 and sim_visits[p, :] = 0: the budget of a move starts.
 * PCBENV_GUMBEL_ABSORB.  pcbenv_puct_advance's PCBENV_TREE_ABSORB, word for word: the same fields, the same all-or-nothing
 * expansion, the same error bits (bit 0, value 1: the children did not fit; bit 1, value 2: selected, num_nodes or a
 * parent out of range).
 * PCBENV_GUMBEL_SELECT.  Start at node 0.  A root that is terminal or has k == 0 gives selected = 0 and path_len = 0 and
 * consumes no simulation; a root whose child range fails the check gives the same and ORs bit 1 into *errors_dev.
 * Otherwise read t = sim_index[p].  t < 0: bit 1 is ORed into *errors_dev, selected = 0, path_len = 0 and nothing else is
 * stored.  t >= n: level 0 is chosen by pcbenv_puct_advance's rule like any other level, and the counters are untouched.
 * Otherwise let v = considered[m * n + t] and S = the children with sim_visits[p, c] == v, or all k children if there is
 * none; c* = the argmax of score_c over S, ties to the lowest c; sim_visits[p, c*] += 1, sim_index[p] = t + 1, paths[0, p,
 * :] = node_action(fc + c*).  Levels d >= 1 are pcbenv_puct_advance's SELECT exactly, at most T levels in all.  SELECT
 * stores only selected, path_len, the path rows it takes, sim_index[p] and one element of sim_visits; it never stores to
 * the tree.
 * The table.  considered int32 [Mc + 1, n], row m for m candidates and n simulations: the considered visit count of
 * simulation t.  Row 0 is zeros; row 1 is 0, 1, ..., n - 1; otherwise, with e the least integer with 2^e >= m, visits[0 ..
 * m) = 0 and nc = m, repeat until n entries exist: extra = max(1, n / (e * nc)) in integer division; extra times, append
 * visits[0 .. nc) and add 1 to each of them; nc = max(2, nc / 2).  (m, n) = (4, 8) gives 0 0 0 0 1 1 2 2.  The kernel only
 * compares a table entry with a counter, it never addresses with one (pcbenv/search.py:considered_visits builds it).
 * PCBENV_GUMBEL_CHOOSE.  A root with k == 0, or one whose child range fails the check (which also ORs bit 1 into
 * *errors_dev), gets move_slot = -1, move_action = 0 and zeros in child_weights, child_policy and child_actions.
 * Otherwise vmax = max_c sim_visits[p, c], S = the children at vmax, c* = the argmax of score_c over S, ties to the lowest
 * c; move_slot = fc + c* and move_action = node_action(fc + c*).  The policy target: x_c = logit_c + sigma_c, mx = their
 * maximum, e_c = exp(x_c - mx), Z = e_0 + e_1 + ... + e_(k-1) summed in that order, pi_c = e_c / Z; child_policy[p, c] =
 * (float)pi_c, child_weights[p, c] = (int32)(pi_c * 16777216.0 + 0.5), entries behind k are zero.  child_actions[p, c] =
 * node_action(fc + c), zero behind k, and root_value[p] = value_sum(0) / visits(0), as pcbenv_puct_move's CHOOSE writes
 * them.  Every element of the six outputs is written.  child_weights has the dtype and layout of pcbenv_puct_move's
 * child_visits: pcbenv_evaluate_visits reads it as it is, because it divides by the integer sum.  CHOOSE stores nothing
 * else.
 * Layouts (int32 unless said): the tree and exchange tensors as in pcbenv_search.h; sim_index [P]; sim_visits [P, C];
 * considered [Mc + 1, n]; move_slot [P]; move_action [P, 3]; child_weights [P, C]; child_policy float32 [P, C];
 * child_actions [P, C, 3]; root_value float64 [P].  errors_dev may be NULL.
 * PCBENV_EINVAL (checked before any device call, in this order): null request; struct_size not
 * sizeof(pcbenv_gumbel_request); phases 0 or with unknown bits, then CHOOSE together with SELECT; num_roots < 0; capacity
 * < 1; max_children outside [1, PCBENV_MAX_TREE_CHILDREN]; max_steps < 1; num_candidates < 1 (ABSORB); num_simulations <
 * 1; max_considered outside [1, 64]; reserved != 0; c_visit or c_scale not finite or negative; a null tensor among
 * num_nodes ... reward_hi (every phase); null sim_index or sim_visits (BEGIN, SELECT, CHOOSE); null selected (ABSORB,
 * SELECT); null path_len, paths or considered (SELECT); null value, leaf_terminal, cand_count, cand_actions or cand_prior
 * (ABSORB); null move_slot, move_action, child_weights, child_policy, child_actions or root_value (CHOOSE); a float64
 * tensor not 8-byte aligned; cand_prior (ABSORB) or child_policy (CHOOSE) not 4-byte aligned; null handle.  num_roots == 0
 * is a no-op success. */
typedef struct pcbenv_gumbel_request {
    uint32_t struct_size; int32_t phases;            /* BEGIN, ABSORB, SELECT, CHOOSE in that order; SELECT|CHOOSE is EINVAL */
    int32_t num_roots /*P*/, capacity /*N node slots per root*/, max_children /*C*/, max_steps /*T*/, num_candidates /*K*/;
    int32_t num_simulations /*n*/, max_considered /*Mc*/, first_root /*global index of root 0 in the draw hash*/, reserved /*0*/;
    double c_puct, c_visit, c_scale;
    uint64_t seed, step_index;                       /* of the Gumbel draws */
    /* the tree, caller-owned device memory, root-major */
    int32_t *num_nodes;                              /* [P] */
    int32_t *parent, *depth, *visits, *num_children, *first_child; /* [P, N] */
    int32_t *node_action;                            /* [P, N, 3] */
    double *prior, *value_sum, *value_max;           /* [P, N] */
    uint8_t *terminal;                               /* [P, N] */
    double *reward_lo, *reward_hi;                   /* [P] */
    /* exchange with the evaluator (tuple format, step-major) */
    int32_t *selected, *path_len;                    /* [P]   written by SELECT */
    int32_t *paths;                                  /* [T, P, 3]: rows t < path_len[p] written, the others untouched */
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
} pcbenv_gumbel_request;
int pcbenv_gumbel_advance(const pcbenv *env, const pcbenv_gumbel_request *req);

#ifdef __cplusplus
}
#endif
#endif /* PCBENV_GUMBEL_H */
