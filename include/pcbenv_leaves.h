/* pcbenv_leaves.h -- leaf-parallel PUCT search on the device, beyond include/pcbenv.h: pcbenv_puct_advance_leaves, the
 * tree step of pcbenv_puct_advance with several leaves per root and launch.  An addition next to pcbenv.h,
 * pcbenv_search.h, pcbenv_priors.h and pcbenv_move.h, which stay as they are: the ABI version is pcbenv.h's and is
 * unchanged, libpcbenv.so exports the entry point below as well, and pcbenv/_leaves_lib.py binds it.
 *
 * Streams.  As pcbenv_puct_advance: the call only enqueues one kernel on its request's stream.
 *
 * What it replaces: nothing in the reference, which has no search.  With one leaf per root an evaluator sees P nodes at
 * a time, P the number of games; with L leaves it sees P * L, and one launch backs all of them up.
 */
#ifndef PCBENV_LEAVES_H
#define PCBENV_LEAVES_H

#include "pcbenv_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCBENV_MAX_PUCT_LEAVES 64

/* pcbenv_puct_advance (pcbenv_search.h) with L = num_leaves leaves per root: SELECT descends every tree L times before
 * anything is evaluated, every descent leaving a pending (virtual) visit on its path so that the next one goes
 * elsewhere, and ABSORB backs all of them up -- P search trees, one per root, in one kernel launch on req->stream.  The
 * caller owns every tensor; the handle supplies the device and pcbenv_last_error only: nothing the library owns is read
 * or written and no bound buffers are needed.  Enqueue only, no allocation, no synchronisation, one kernel on
 * req->stream.  Not meant to be captured into a hipGraph.
 * The tree is pcbenv_puct_request's (same names, dtypes and layouts: N = capacity slots per root, a node's k <= C =
 * max_children children in the slots first_child .. first_child + k - 1) and one tensor more: pending int32 [P, N], the
 * visits selected but not yet absorbed.  The exchange tensors have a leaf extent, root-major: row r = p * L + l is leaf
 * l of root p, the order of pcbenv_playout's k playouts per root.
 * phases is a set of PCBENV_TREE_INIT, PCBENV_TREE_ABSORB, PCBENV_TREE_SELECT (pcbenv.h); one launch runs them in the
 * order INIT, ABSORB, SELECT.
 * PCBENV_TREE_INIT.  What pcbenv_puct_advance's INIT does, and pending = 0 in every slot.
 * PCBENV_TREE_SELECT.  For l = 0 .. L - 1, in that order, one descent as pcbenv_puct_advance's SELECT makes it -- from
 * node 0, while d < max_steps, stopping at a node that is terminal or has num_children == 0, the child range checked,
 * ties go to the lowest c -- with the score of child ch = fc + c of `node`
 *   n_c = (double)(visits(ch) + pending(ch)),
 *   q = (visits(ch) > 0 && reward_hi > reward_lo)
 *         ? ((value_sum(ch) / (double)visits(ch) - reward_lo) / (reward_hi - reward_lo)) * ((double)visits(ch) / n_c) : 0,
 *   u = c_puct * prior(ch) * sqrt((double)max(visits(node) + pending(node), 1)) / (1.0 + n_c),
 * score = q + u: all of it float64, one IEEE operation per operator, evaluated left to right, the two sums formed in 64
 * bits.  No logarithm is computed.  A pending visit counts as a visit that returned reward_lo; with pending == 0 the
 * factor visits / n_c is exactly 1.0 and the score is pcbenv_puct_advance's bit for bit.  The descent of leaf l reads
 * pending as the leaves before it left it.
 * A repeat is a descent that ends at a node that is not terminal, has no children and has pending > 0 already: every
 * later descent of the launch would end there too.  The selection of that root stops: selected[r] = path_len[r] = -1 for
 * this and all later leaves of the root, and the repeat adds no pending visit.  The repeat's own path rows d < the levels
 * it took hold the actions it passed (those of the earlier leaf that ended there); the path rows of the leaves behind it
 * are untouched.  Any other descent writes selected[r] = the node reached, path_len[r] = the levels taken, paths[d, r, :]
 * = node_action of the node entered at level d for d < path_len[r] -- rows >= path_len[r] are untouched -- and adds 1
 * to pending of every node of the descent, the root and the node reached included.  A terminal node may be selected more
 * than once.  At most max_steps levels per descent.
 * PCBENV_TREE_ABSORB.  For l = 0 .. L - 1, in that order, with r = p * L + l: selected[r] == -1 skips the leaf, and none
 * of that row's inputs is read.  Otherwise value[r], leaf_terminal[r], cand_count[r], cand_actions[r, :, :] and
 * cand_prior[r, :] describe the node selected[r], and the leaf is absorbed exactly as pcbenv_puct_advance's ABSORB
 * absorbs its one: the terminal mark, which is never cleared; the expansion with k = clamp(cand_count, 0, min(K, C))
 * children, all or nothing, bit 0 (value 1) of *errors_dev if they do not fit; reward_lo and reward_hi; visits += 1,
 * value_sum += value, value_max = max(value_max, value) on the node and every ancestor, at most max_steps + 1 nodes --
 * and pending -= 1 on each of those nodes.  After ABSORB has taken every leaf of a SELECT, pending is zero everywhere and
 * the tree is one pcbenv_puct_advance and pcbenv_puct_move take unchanged.
 * A SELECT that follows a SELECT without an ABSORB between them adds to the pending visits that are there: the caller
 * pairs every SELECT with the ABSORB of its leaves.
 * A slot number or count the kernel reads back -- selected[r], num_nodes[p], a node's first_child and num_children, a
 * parent -- is compared with N or C before it addresses anything; one out of range ORs bit 1 (value 2) into *errors_dev.
 * In SELECT the descent ends there and is written as it stands, and the next leaf follows; in ABSORB -- selected[r]
 * outside [-1, N), num_nodes outside [1, N], a parent outside [-1, N) -- that root's phase ends.  pending is data: it
 * never addresses anything, whatever it holds.
 * Layouts (int32 unless said): the tree as in pcbenv_puct_request; pending [P, N]; selected, path_len [P * L]; paths
 * [T, P * L, 3], step-major, T = max_steps; value float64 [P * L]; leaf_terminal uint8 [P * L]; cand_count [P * L];
 * cand_actions [P * L, K, 3]; cand_prior float32 [P * L, K].  errors_dev may be NULL.
 * PCBENV_EINVAL (checked before any device call, in this order): null request; struct_size not
 * sizeof(pcbenv_puct_leaves_request); phases 0 or with unknown bits, then INIT together with ABSORB; num_roots < 0;
 * capacity < 1; max_children outside [1, PCBENV_MAX_TREE_CHILDREN]; max_steps < 1; num_leaves outside
 * [1, PCBENV_MAX_PUCT_LEAVES]; num_roots * num_leaves above 2^31 - 1; num_candidates < 1 (ABSORB); reserved or reserved2
 * != 0; a null tensor among num_nodes ... reward_hi and pending (every phase); null selected (ABSORB, SELECT); null
 * path_len or paths (SELECT); null value, leaf_terminal, cand_count, cand_actions or cand_prior (ABSORB); a float64 tensor
 * not 8-byte aligned or cand_prior not 4-byte aligned; null handle.  num_roots == 0 is a no-op success. */
typedef struct pcbenv_puct_leaves_request {
    uint32_t struct_size; int32_t phases;            /* INIT, ABSORB, SELECT in that order; INIT|ABSORB is EINVAL */
    int32_t num_roots /*P*/, capacity /*N node slots per root*/, max_children /*C*/, max_steps /*T*/, num_candidates /*K*/, reserved /*0*/;
    double c_puct;
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
    uint32_t *errors_dev;                            /* optional */
    void *stream;
} pcbenv_puct_leaves_request;
int pcbenv_puct_advance_leaves(const pcbenv *env, const pcbenv_puct_leaves_request *req);

#ifdef __cplusplus
}
#endif
#endif /* PCBENV_LEAVES_H */
