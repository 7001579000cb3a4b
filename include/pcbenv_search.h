/* pcbenv_search.h -- search on the device that goes beyond include/pcbenv.h: pcbenv_puct_advance, the tree of a batched
 * PUCT (AlphaZero-style) search.  An addition next to pcbenv.h, which stays as it is: PCBENV_ABI_VERSION is unchanged,
 * libpcbenv.so exports the entry point below as well, and pcbenv/_search_lib.py binds it.
 *
 * Streams.  As pcbenv_tree_advance: the call only enqueues one kernel on its request's stream.
 *
 * What it replaces: nothing in the reference, which has no search.  It is the bookkeeping of a batched PUCT around a
 * network: pcbenv_gather_paths materialises the node a path names so that a policy can score it, and this call keeps the
 * tree -- priors in selection and expansion, a value instead of a playout at the leaf.
 */
#ifndef PCBENV_SEARCH_H
#define PCBENV_SEARCH_H

#include "pcbenv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tree of a PUCT search around an evaluator: selection with priors, expansion of a node with all its children at
 * once, and backup of P search trees, one per root, in one kernel launch on req->stream.  An iteration of a batched
 * search is then the caller's evaluation of the P nodes that selected / path_len / paths name (pcbenv_gather_paths and a
 * network, or pcbenv_playout_paths) and one pcbenv_puct_advance(ABSORB | SELECT) that absorbs it and writes the next
 * selection.  The caller owns every tensor; the handle supplies the device and pcbenv_last_error only: nothing the
 * library owns is read or written and no bound buffers are needed.  Enqueue only, no allocation, no synchronisation.
 * Not meant to be captured into a hipGraph.
 * The tree of root p has N = capacity node slots, slot 0 the root.  A node is expanded once, with all its k <= C =
 * max_children children at once: they take the consecutive slots first_child .. first_child + k - 1.
 * phases is a set of PCBENV_TREE_INIT, PCBENV_TREE_ABSORB, PCBENV_TREE_SELECT (pcbenv.h); one launch runs them in the
 * order INIT, ABSORB, SELECT.
 * PCBENV_TREE_INIT.  num_nodes = 1, reward_lo = +inf, reward_hi = -inf; every slot (the root and the unused ones
 * alike): parent = -1, first_child = -1, depth = 0, visits = 0, num_children = 0, node_action = 0, prior = 0,
 * value_sum = 0, value_max = -inf, terminal = 0.
 * PCBENV_TREE_SELECT.  Start at node 0, level d = 0.  While d < max_steps: stop at a node that is terminal or has
 * num_children == 0; otherwise, with fc = first_child(node) and k = num_children(node), go to the child ch = fc + c,
 * c < k, with the highest score = q + u,
 *   q = (n_c > 0 && reward_hi > reward_lo) ? (value_sum(ch) / n_c - reward_lo) / (reward_hi - reward_lo) : 0,
 *   u = c_puct * prior(ch) * sqrt((double)max(visits(node), 1)) / (1.0 + n_c),   n_c = visits(ch);
 * all of it float64, one IEEE operation per operator, evaluated left to right; ties go to the lowest c.  No logarithm is
 * computed, so there is no table.  Level d of the descent writes paths[d, p, :] = node_action(ch); at the end
 * selected[p] = the node reached and path_len[p] = the levels taken.  Rows >= path_len[p] of paths are untouched.  At
 * most max_steps levels.
 * PCBENV_TREE_ABSORB.  value[p], leaf_terminal[p], cand_count[p], cand_actions[p, :, :], cand_prior[p, :] describe
 * the node selected[p] as the caller evaluated it (values are finite).  With node = selected[p]: if leaf_terminal,
 * terminal(node) = 1; it is never cleared.  Else, if num_children(node) == 0 and the node is not terminal, k =
 * clamp(cand_count, 0, min(K, C)), K = num_candidates -- a count out of range is data, not an error -- and if k > 0 and
 * num_nodes + k <= N the slots num_nodes .. num_nodes + k - 1 become the children: parent = node, depth = depth(node) +
 * 1, node_action = cand_actions[p, c], prior = cand_prior[p, c] widened exactly to float64; first_child(node) =
 * num_nodes, num_children(node) = k, num_nodes += k.  If they do not fit none is made, all or nothing, and bit 0
 * (value 1) is ORed into *errors_dev.  Priors are used as given: they are not renormalised over the k kept.  Then
 * reward_lo = min(reward_lo, value), reward_hi = max(reward_hi, value); visits += 1, value_sum += value, value_max =
 * max(value_max, value) on the node and every ancestor, at most max_steps + 1 nodes.
 * A slot number or count the kernel reads back -- selected[p], num_nodes[p], a node's first_child and num_children
 * (1 <= fc, 1 <= k <= C and fc + k <= N are required of an expanded node), a parent -- is compared with N or C before it
 * addresses anything; one out of range ends that root's phase where it stands and ORs bit 1 (value 2) into *errors_dev.
 * Layouts (int32 unless said): num_nodes [P]; parent, depth, visits, num_children, first_child [P, N]; node_action
 * [P, N, 3]; prior, value_sum, value_max float64 [P, N]; terminal uint8 [P, N]; reward_lo, reward_hi float64 [P];
 * selected, path_len [P]; paths [T, P, 3] -- the step-major tuple format of pcbenv_playout_paths' and
 * pcbenv_gather_paths' path_actions_dev, T = max_steps; value float64 [P]; leaf_terminal uint8 [P]; cand_count [P];
 * cand_actions [P, K, 3]; cand_prior float32 [P, K].  errors_dev may be NULL.
 * PCBENV_EINVAL (checked before any device call, in this order): null request; struct_size not
 * sizeof(pcbenv_puct_request); phases 0 or with unknown bits, then INIT together with ABSORB; num_roots < 0; capacity < 1;
 * max_children outside [1, PCBENV_MAX_TREE_CHILDREN]; max_steps < 1; num_candidates < 1 (ABSORB); reserved != 0; a null
 * tensor among num_nodes ... reward_hi (every phase); null selected (ABSORB, SELECT); null path_len or paths (SELECT);
 * null value, leaf_terminal, cand_count, cand_actions or cand_prior (ABSORB); a float64 tensor not 8-byte aligned or
 * cand_prior not 4-byte aligned; null handle.  num_roots == 0 is a no-op success. */
typedef struct pcbenv_puct_request {
    uint32_t struct_size; int32_t phases;            /* INIT, ABSORB, SELECT in that order; INIT|ABSORB is EINVAL */
    int32_t num_roots /*P*/, capacity /*N node slots per root*/, max_children /*C*/, max_steps /*T*/, num_candidates /*K*/, reserved /*0*/;
    double c_puct;
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
    uint32_t *errors_dev;                            /* optional */
    void *stream;
} pcbenv_puct_request;
int pcbenv_puct_advance(const pcbenv *env, const pcbenv_puct_request *req);

#ifdef __cplusplus
}
#endif
#endif /* PCBENV_SEARCH_H */
