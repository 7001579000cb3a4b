/* pcbenv_frontier.h -- a beam search over placements on the device, beyond include/pcbenv.h: pcbenv_frontier_advance, the
 * frontier step of such a search.  (pcbenv.h's "beam" is the net search of the routing reward; the set of partial
 * placements a search over placements keeps per depth is called a frontier everywhere in code.)  An addition next to
 * pcbenv.h, pcbenv_search.h, pcbenv_priors.h, pcbenv_move.h and pcbenv_leaves.h, which stay as they are: the ABI version
 * is pcbenv.h's and is unchanged, libpcbenv.so exports the entry point below as well, and pcbenv/_frontier_lib.py binds it.
 *
 * Streams.  As pcbenv_puct_advance: the call only enqueues one kernel on its request's stream.
 *
 * What it replaces: nothing in the reference, which has no search.  Placement is a deterministic construction in a fixed
 * order with its reward at the end; per root, a frontier of W partial placements is expanded by the K best legal actions
 * of each, the W * K children are evaluated, and the W best of them are the next frontier.
 */
#ifndef PCBENV_FRONTIER_H
#define PCBENV_FRONTIER_H

#include "pcbenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCBENV_FRONTIER_INIT 1
#define PCBENV_FRONTIER_ADVANCE 2
#define PCBENV_MAX_FRONTIER_WIDTH 64
#define PCBENV_MAX_FRONTIER_CANDIDATES 64
#define PCBENV_MAX_FRONTIER_ROWS 1024

/* One depth of P beam searches over placements, one per root, in one kernel launch on req->stream.  The caller owns every
 * tensor; the handle supplies the device and pcbenv_last_error only: nothing the library owns is read or written and no
 * bound buffers are needed.  Enqueue only, no allocation, no synchronisation, one kernel on req->stream.  Not meant to be
 * captured into a hipGraph.
 * Sizes: W = width, K = num_candidates, F = W * K rows per root, T = max_steps.  Row r = p * F + i is slot i of root p,
 * root-major as the leaf rows of pcbenv_puct_advance_leaves.  A row is a partial placement named by its path: paths
 * [T, P * F, 3] step-major, the layout pcbenv_gather_paths and pcbenv_playout_paths take, path_len [P * F] with -1 = no
 * row, cum_logp float64 [P * F].  There are two such sets, `in` and `out`, which the caller swaps between calls.
 * phases is PCBENV_FRONTIER_INIT or PCBENV_FRONTIER_ADVANCE; both in one request is PCBENV_EINVAL.
 * PCBENV_FRONTIER_INIT writes the out set and nothing else: path_len_out = 0 for slot 0 of every root and -1 for the
 * others, cum_logp_out of slot 0 = 0.0, parent_row = -1, live = 1, best_len = -1 and best_value = -inf.  paths_out and
 * best_path are untouched.
 * PCBENV_FRONTIER_ADVANCE, for root p, reads the in set and the evaluation of its rows -- value[r], leaf_terminal[r],
 * cand_count[r], cand_actions[r, :, :], cand_prior[r, :], what pcbenv_puct_advance_leaves' ABSORB takes -- writes the out
 * set, and updates best_value, best_len and best_path.  Four steps.
 * (1) Live rows.  A row is live if path_len_in[r] is in [0, T].  A value outside [-1, T] makes the row no row and ORs bit 1
 * (value 2) into *errors_dev.  Of a row that is not live nothing else is read.
 * (2) Finished rows.  Live rows with leaf_terminal[r] != 0 are finished.  They are taken in increasing i, with v =
 * value[r] and a NaN counted as -inf: if best_len[p] == -1 or v > best_value[p] (strictly greater, as doubles), then
 * best_value[p] = v, best_len[p] = path_len_in[r] and best_path[d, p, :] = paths_in[d, r, :] for d < that length, later
 * rows untouched.  A finished row is never expanded.
 * (3) The order of the expandable rows.  Live, unfinished rows are expandable if path_len_in[r] < T and k_r =
 * clamp(cand_count[r], 0, K) > 0; the others are dropped without an error (a count is data, as in PUCT's ABSORB).  The
 * score of an expandable row is s = value[r] if prior_weight == 0 -- cum_logp is then not read into the score, so no
 * 0 * inf arises -- and s = value[r] + prior_weight * cum_logp_in[r] otherwise: float64, two IEEE operations, no
 * contraction.  A NaN counts as -inf.  The order is s descending, as doubles, so -0.0 ties with +0.0, and ties go to the
 * lower i.  The first n = min(W, number expandable) rows are kept.  The kept row of rank w is i_w.
 * (4) The children.  The children of rank w go to slots w * K + c, c < k.  For each: paths_out[d, row, :] =
 * paths_in[d, parent, :] for d < len, and paths_out[len, row, :] = cand_actions[parent, c, :]; later path rows are
 * untouched.  path_len_out = len + 1.  cum_logp_out = cum_logp_in[parent] + lp, with lp = ln((double)prior), the
 * logarithm in IEEE + - * / alone that the root noise uses, if the prior is a positive, finite, normal float32, and -inf
 * otherwise.  parent_row = i_w.  Every other slot of the root gets path_len_out = -1 and parent_row = -1; its
 * cum_logp_out and path rows are untouched.  live[p] is the number of child rows written.
 * Candidate actions are data.  They are copied, never used as an index, and a bad one ends its row's episode in the
 * evaluator as a bad path action does everywhere else.
 * A search is INIT, then per depth d the evaluation of (paths_out, path_len_out) with step index step_index + d * T
 * followed by ADVANCE with the sets swapped: T + 1 evaluations at most, no host synchronisation, and rows of -1 cost the
 * evaluator nothing.  With prior_weight = 0 it is a beam search by value; with a constant value and prior_weight = 1 it
 * is the classic beam search by cumulative log-probability.
 * Layouts (int32 unless said): paths_in, paths_out [T, P * F, 3]; path_len_in, path_len_out [P * F]; cum_logp_in,
 * cum_logp_out float64 [P * F]; parent_row [P * F], the slot i of the parent in the input frontier, -1 for no row; live
 * [P]; best_value float64 [P]; best_len [P]; best_path [T, P, 3]; value float64 [P * F]; leaf_terminal uint8 [P * F];
 * cand_count [P * F]; cand_actions [P * F, K, 3]; cand_prior float32 [P * F, K].  errors_dev may be NULL.
 * PCBENV_EINVAL (checked before any device call, in this order): null request; struct_size not
 * sizeof(pcbenv_frontier_request); phases 0 or with unknown bits, then INIT together with ADVANCE; num_roots < 0; width
 * outside [1, PCBENV_MAX_FRONTIER_WIDTH]; num_candidates outside [1, PCBENV_MAX_FRONTIER_CANDIDATES]; width *
 * num_candidates above PCBENV_MAX_FRONTIER_ROWS; max_steps < 1; num_roots * width * num_candidates above 2^31 - 1;
 * prior_weight NaN or infinite; reserved or reserved2 != 0; a null tensor among paths_out, path_len_out, cum_logp_out,
 * parent_row, live, best_value, best_len (every phase); a null tensor among paths_in, path_len_in, cum_logp_in, best_path,
 * value, leaf_terminal, cand_count, cand_actions, cand_prior (ADVANCE); a float64 tensor not 8-byte aligned or cand_prior
 * not 4-byte aligned; with ADVANCE, the bytes of paths_in, path_len_in or cum_logp_in overlapping those of its out twin;
 * null handle.  num_roots == 0 is a no-op success. */
typedef struct pcbenv_frontier_request {
    uint32_t struct_size; int32_t phases;            /* INIT or ADVANCE; both is EINVAL */
    int32_t num_roots /*P*/, width /*W*/, num_candidates /*K*/, max_steps /*T*/;
    double prior_weight;
    int32_t reserved /*0*/, reserved2 /*0*/;
    /* the two sets of frontier rows, caller-owned device memory, row r = p * W * K + i */
    const int32_t *paths_in, *path_len_in; const double *cum_logp_in;   /* read by ADVANCE */
    int32_t *paths_out, *path_len_out; double *cum_logp_out;            /* written by INIT (not paths_out) and ADVANCE */
    int32_t *parent_row;                             /* [P * F] */
    int32_t *live;                                   /* [P] */
    double *best_value; int32_t *best_len;           /* [P]   read and written by every ADVANCE */
    int32_t *best_path;                              /* [T, P, 3] */
    const double *value; const uint8_t *leaf_terminal; const int32_t *cand_count, *cand_actions; const float *cand_prior; /* read by ADVANCE */
    uint32_t *errors_dev;                            /* optional */
    void *stream;
} pcbenv_frontier_request;
int pcbenv_frontier_advance(const pcbenv *env, const pcbenv_frontier_request *req);

#ifdef __cplusplus
}
#endif
#endif /* PCBENV_FRONTIER_H */
