/* pcbenv_frontier_sample.h -- stochastic beam search over placements on the device, beyond include/pcbenv.h:
 * pcbenv_frontier_sample, the frontier step of pcbenv_frontier.h with the rows ordered by Gumbel-perturbed cumulative
 * log-probabilities drawn top-down (Kool, van Hoof and Welling, "Stochastic Beams and Where to Find Them", ICML 2019).  An
 * addition next to pcbenv.h, pcbenv_search.h, pcbenv_priors.h, pcbenv_move.h, pcbenv_leaves.h and pcbenv_frontier.h, which
 * stay as they are: the ABI version is pcbenv.h's and is unchanged, libpcbenv.so exports the entry point below as well, and
 * pcbenv/_frontier_sample_lib.py binds it.
 *
 * Streams.  As pcbenv_frontier_advance: the call only enqueues one kernel on its request's stream.
 *
 * What it replaces: nothing in the reference, which has no search.  pcbenv_frontier_advance returns one plan per root,
 * always the same one; this step returns W complete placements per root sampled without replacement from the policy, in
 * Plackett-Luce order, each with its value and its log-probability.
 */
#ifndef PCBENV_FRONTIER_SAMPLE_H
#define PCBENV_FRONTIER_SAMPLE_H

#include "pcbenv_frontier.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One depth of P stochastic beam searches over placements, one per root, in one kernel launch on req->stream.  The caller
 * owns every tensor; the handle supplies the device and pcbenv_last_error only.  Enqueue only, no allocation, no
 * synchronisation, one kernel on req->stream.  Not meant to be captured into a hipGraph.
 * Sizes, rows, the two sets `in` and `out`, the phases (PCBENV_FRONTIER_INIT or PCBENV_FRONTIER_ADVANCE; both in one
 * request is PCBENV_EINVAL), the evaluation tensors and the bounds are pcbenv_frontier.h's: W = width, K =
 * num_candidates, F = W * K rows per root, T = max_steps, row r = p * F + i is slot i of root p.  A set has a third
 * member, gumbel float64 [P * F]: the perturbed log-probability G of a row.  Beside the rows a root has a sample set of W
 * slots, slot p * W + j: set_len [P * W] with -1 for a free slot, set_gumbel, set_logp, set_value float64 [P * W], and
 * set_path [T, P * W, 3] step-major.
 * PCBENV_FRONTIER_INIT does what pcbenv_frontier_advance's INIT does -- path_len_out = 0 for slot 0 of every root and -1
 * for the others, cum_logp_out of slot 0 = 0.0, parent_row = -1, live = 1, best_len = -1, best_value = -inf -- and in
 * addition gumbel_out of slot 0 = 0.0 and set_len = -1 everywhere.  paths_out, best_path and the other set tensors are
 * untouched.
 * PCBENV_FRONTIER_ADVANCE, for root p, in five steps.
 * (1) Live rows.  As pcbenv_frontier_advance step 1: a row is live if path_len_in[r] is in [0, T], a value outside [-1, T]
 * is no row and ORs bit 1 (value 2) into *errors_dev, and of a row that is not live nothing else is read.
 * (2) Best finished row.  As its step 2: the live rows with leaf_terminal[r] != 0 compete, in increasing i, for best_value,
 * best_len and best_path by value, a NaN counted as -inf, strictly greater winning.  A finished row is never expanded.
 * (3) The contenders.  The key of a contender is its G with a NaN counted as -inf; the value is never read into a key.
 * Set slots j < W are contenders with key set_gumbel[p * W + j] if set_len is in [0, T] (an entry); a set_len outside
 * [-1, T] is no entry and ORs bit 2 (value 4) into *errors_dev.  The live rows that are finished or expandable
 * (expandable as in pcbenv_frontier_advance step 3: unfinished, path_len_in < T, clamp(cand_count, 0, K) > 0) are
 * contenders with key gumbel_in[r]; live rows that are neither are dropped without an error.
 * (4) The winners.  One total order covers all contenders: the key descending, as doubles, so -0.0 ties with +0.0, and ties
 * go to the lower id, the id being j for a set slot and W + i for row i: on equal keys a set entry goes before a row.  The
 * first min(W, contenders) are the winners.  Set entries that did not win get set_len = -1 and nothing else.  Finished
 * rows that won enter the set in rank order, the m-th into the m-th lowest slot that is not a surviving entry (there are
 * always enough): set_len = path_len_in[r], set_gumbel = its key, set_logp = cum_logp_in[r], set_value = value[r] and
 * set_path[d, slot, :] = paths_in[d, r, :] for d < len, the last three copied as data, later path rows untouched.
 * Expandable rows that won are the kept parents, i_w the one of rank w among them, n <= W of them.
 * (5) The children.  As pcbenv_frontier_advance step 4 -- slots w * K + c, paths_out, path_len_out = len + 1, cum_logp_out =
 * cum_logp_in[parent] + ln(prior) or -inf, parent_row = i_w, every other slot path_len_out = parent_row = -1 and nothing
 * else, live[p] the number of child rows written -- plus gumbel_out of every child row.  With G_S the key of the parent,
 * phi_c = cum_logp_out of child c, g_c = -ln(-ln u) for u = draw number 256 + i_w of child c in the uniform stream of
 * pcbenv_puct_root_noise for (seed, first_root + p, step_index) -- 256 lies above every draw number the root noise (0 to
 * 96) and the Gumbel searches (128) use -- G_c = phi_c + g_c and Z the largest G_c over the children with finite phi_c,
 * gumbel_out of child c is
 *   -inf                                            if phi_c is not finite,
 *   G_S, copied                                     if G_S is not finite,
 *   G_S                                             if a == 0 or d <= 0, where a = G_c - Z, e = exp(a), d = 1 - e,
 *   (G_S - max(v, 0)) - ln(1 + exp(-|v|))           otherwise, with v = (G_S - G_c) + ln d.
 * Every ln and exp is the one in IEEE + - * / alone that the root noise uses, one IEEE operation per written operator, no
 * contraction.  Their arguments lie inside those functions' domains by the arms above: a <= 0 and -|v| <= 0 (an infinite
 * one gives exp = 0 exactly), u and -ln u are positive normal numbers, d is in [2^-53, 1] behind d <= 0, and 1 + exp(-|v|)
 * is in [1, 2]; no further guard is needed.
 * What these give.  Exact maximum: the largest gumbel_out among a parent's children equals the parent's G bit for bit and
 * no child exceeds it.  Final set: when a search has run until live == 0, the set entries in descending set_gumbel are an
 * ordered sample without replacement of complete placements from the policy restricted, at every node, to the K
 * candidates the evaluator gave, and the first is an exact sample of that policy renormalised at every node.  The
 * candidates of the root need not sum to 1, a common factor cancels; below the root the later entries are exact when every
 * node's candidates sum to 1, as they do when K covers the legal actions, and under-weight the siblings of earlier entries
 * where they sum to less.  Dropped entries stay out: no G written later exceeds its parent's, and W contenders went
 * before the dropped one, so a dropped set entry can never have come back, which is why dropping it is exact.  Batch
 * independence: a draw depends on (seed, global root, step_index, i_w, c) alone, not on the batch.
 * A search is INIT, then per depth d the evaluation of (paths_out, path_len_out) followed by ADVANCE with the sets swapped
 * and step_index + d * T, as for pcbenv_frontier_advance.
 * Layouts beyond pcbenv_frontier.h's (int32 unless said): gumbel_in, gumbel_out float64 [P * F]; set_len [P * W];
 * set_gumbel, set_logp, set_value float64 [P * W]; set_path [T, P * W, 3].  errors_dev may be NULL.
 * PCBENV_EINVAL (checked before any device call, in this order): null request; struct_size not
 * sizeof(pcbenv_frontier_sample_request); phases 0 or with unknown bits, then INIT together with ADVANCE; num_roots < 0;
 * width outside [1, PCBENV_MAX_FRONTIER_WIDTH]; num_candidates outside [1, PCBENV_MAX_FRONTIER_CANDIDATES]; width *
 * num_candidates above PCBENV_MAX_FRONTIER_ROWS; max_steps < 1; num_roots * width * num_candidates above 2^31 - 1;
 * first_root < 0 or first_root + num_roots above 2^31 - 1; reserved != 0; a null tensor among paths_out, path_len_out,
 * cum_logp_out, gumbel_out, parent_row, live, best_value, best_len, set_len, set_gumbel, set_logp, set_value, set_path
 * (every phase); a null tensor among paths_in, path_len_in, cum_logp_in, gumbel_in, best_path, value, leaf_terminal,
 * cand_count, cand_actions, cand_prior (ADVANCE); a float64 tensor not 8-byte aligned or cand_prior not 4-byte aligned;
 * with ADVANCE, the bytes of paths_in, path_len_in, cum_logp_in or gumbel_in overlapping those of its out twin; null
 * handle.  num_roots == 0 is a no-op success. */
typedef struct pcbenv_frontier_sample_request {
    uint32_t struct_size; int32_t phases;            /* INIT or ADVANCE; both is EINVAL */
    int32_t num_roots /*P*/, width /*W*/, num_candidates /*K*/, max_steps /*T*/;
    uint64_t seed, step_index;
    int32_t first_root /*the global index of root 0*/, reserved /*0*/;
    /* the two sets of frontier rows, caller-owned device memory, row r = p * W * K + i */
    const int32_t *paths_in, *path_len_in; const double *cum_logp_in, *gumbel_in;   /* read by ADVANCE */
    int32_t *paths_out, *path_len_out; double *cum_logp_out, *gumbel_out;           /* written by INIT (not paths_out) and ADVANCE */
    int32_t *parent_row;                             /* [P * F] */
    int32_t *live;                                   /* [P] */
    double *best_value; int32_t *best_len;           /* [P]   read and written by every ADVANCE */
    int32_t *best_path;                              /* [T, P, 3] */
    int32_t *set_len;                                /* [P * W]   written by INIT, read and written by every ADVANCE */
    double *set_gumbel, *set_logp, *set_value;       /* [P * W] */
    int32_t *set_path;                               /* [T, P * W, 3] */
    const double *value; const uint8_t *leaf_terminal; const int32_t *cand_count, *cand_actions; const float *cand_prior; /* read by ADVANCE */
    uint32_t *errors_dev;                            /* optional */
    void *stream;
} pcbenv_frontier_sample_request;
int pcbenv_frontier_sample(const pcbenv *env, const pcbenv_frontier_sample_request *req);

#ifdef __cplusplus
}
#endif
#endif /* PCBENV_FRONTIER_SAMPLE_H */
