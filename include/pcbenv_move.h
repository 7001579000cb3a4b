/* pcbenv_move.h -- the move of a searched game on the device, beyond include/pcbenv.h: pcbenv_puct_move, which picks
 * the move of every root from a PUCT tree and keeps the subtree below it for the next search.  An addition next to
 * pcbenv.h, pcbenv_search.h and pcbenv_priors.h, which stay as they are: the ABI version is pcbenv.h's and is unchanged,
 * libpcbenv.so exports the entry point below as well, and pcbenv/_move_lib.py binds it.
 *
 * Streams.  As pcbenv_puct_advance: the call only enqueues one kernel on its request's stream.
 *
 * What it replaces: nothing in the reference, which has no search.  It is what stands between two searches of a
 * self-play episode: pcbenv/search.py:puct_choose and puct_reroot as one launch each side of the environment's step.
 */
#ifndef PCBENV_MOVE_H
#define PCBENV_MOVE_H

#include "pcbenv_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCBENV_MOVE_CHOOSE 1        /* phases */
#define PCBENV_MOVE_REROOT 2
#define PCBENV_MOVE_GREEDY 0        /* mode */
#define PCBENV_MOVE_PROPORTIONAL 1

/* The move of P PUCT trees (the tree tensors of pcbenv_puct_request, same names, dtypes and layouts), one kernel launch
 * on req->stream.  The caller owns every tensor; the handle supplies the device and pcbenv_last_error only: nothing the
 * library owns is read or written and no bound buffers are needed.  Enqueue only, no allocation, no synchronisation, one
 * kernel on req->stream.  Not meant to be captured into a hipGraph.
 * phases is a set of PCBENV_MOVE_CHOOSE and PCBENV_MOVE_REROOT; one launch runs them in the order CHOOSE, REROOT.  The
 * caller may split them around its environment's step, so that reset can be the done flags that step produced.
 * N = capacity node slots per root, C = max_children.
 * PCBENV_MOVE_CHOOSE.  Let k = num_children(0) and fc = first_child(0).  k == 0: the root has no children.  Otherwise
 * both are checked (1 <= k <= C, 1 <= fc <= N - k) before they address anything; a root that fails is treated as one
 * without children and ORs bit 1 (value 2) into *errors_dev.  child_visits[p, c] = visits(fc + c) and child_actions[p, c]
 * = node_action(fc + c) for c < k; entries behind k are zero.  root_value[p] = value_sum(0) / (double)visits(0): one IEEE
 * division, NaN for an unvisited root.  Every element of the four outputs, of move_slot and of move_action is written.
 * mode == PCBENV_MOVE_GREEDY: the move is the child c* with the most visits, ties to the lowest c.
 * mode == PCBENV_MOVE_PROPORTIONAL: total = the int64 sum of the children's visits; h = hi32(mix64(mix64(seed ^
 * 0x9E3779B97F4A7C15 * (first_root + p + 1)) + step_index)), the draw hash of pcbenv_sample_actions; r = (h * total) >> 32
 * in unsigned 64-bit arithmetic; c* is the least c whose inclusive prefix sum of visits exceeds r.  total <= 0, or no
 * such c, falls back to greedy.  There are no floating-point operations in the choice.
 * move_slot[p] = fc + c* and move_action[p] = that child's action; a root without children gets move_slot = -1 and
 * action (0, 0, 0).
 * PCBENV_MOVE_REROOT.  Let m = move_slot[p] and n = num_nodes[p].
 * reset[p] != 0 (when reset is given) or m == -1: all N slots and the three scalars of the root become exactly what
 * PCBENV_TREE_INIT leaves, whatever the tree held, and remap[p, :] = -1.
 * Otherwise n must be in [1, N] and m in [0, n).  m == 0: the tree is unchanged, remap is the identity on [0, n) and -1
 * behind.  m >= 1: the subtree of m replaces the tree.  A slot s is kept if it is m or its parent is kept; remap[p, s] is
 * the rank of s among the kept slots, in slot order, and -1 for every other slot of the row.  A kept node moves to slot
 * remap[s] and keeps visits, num_children, node_action, prior, value_sum, value_max and terminal; its parent and, where
 * num_children > 0, its first_child go through remap (a node without children has first_child = -1); its depth drops by
 * depth(m).  The new slot 0 has parent = -1, depth = 0, node_action = 0 and prior = 0, as an INIT root has.  num_nodes
 * becomes the number kept, and the slots from there up to n - 1 are given the INIT values; the slots from n on are not
 * written: they hold the INIT values already, as INIT and ABSORB leave every unused slot.  reward_lo and reward_hi are
 * kept: they bound the values seen, and the subtree's are a subset of them.  The compaction runs in place: a parent's
 * slot is below its children's, so no kept node moves up.
 * A damaged tree: every slot number or count read back is compared before it addresses anything.  Required are n in
 * [1, N]; m in [-1, n); 0 <= parent(s) < s for every used s >= 1; of a kept node num_children in [0, C] and, where it is
 * not 0, 1 <= first_child <= n - num_children with every slot of that range kept.  A violation leaves that root's tree
 * tensors untouched -- all or nothing: the tree is validated before the first store to it -- sets its remap row to -1 and
 * ORs bit 1 (value 2) into *errors_dev.
 * Layouts (int32 unless said): the tree as in pcbenv_puct_request; move_slot [P]; move_action [P, 3]; child_visits [P, C];
 * child_actions [P, C, 3]; root_value float64 [P]; remap [P, N]; reset uint8 [P], may be NULL; errors_dev may be NULL.
 * PCBENV_EINVAL (checked before any device call, in this order): null request; struct_size not
 * sizeof(pcbenv_puct_move_request); phases 0 or with unknown bits; unknown mode (CHOOSE); num_roots < 0; capacity < 1;
 * max_children outside [1, PCBENV_MAX_TREE_CHILDREN]; reserved != 0; a null tensor among num_nodes ... reward_hi; null
 * move_slot; null move_action, child_visits, child_actions or root_value (CHOOSE); null remap (REROOT); a float64 tensor
 * not 8-byte aligned; null handle.  num_roots == 0 is a no-op success. */
typedef struct pcbenv_puct_move_request {
    uint32_t struct_size; int32_t phases;            /* CHOOSE, REROOT in that order */
    int32_t num_roots /*P*/, capacity /*N node slots per root*/, max_children /*C*/, mode, first_root /*global index of root 0 in the draw hash*/, reserved /*0*/;
    uint64_t seed, step_index;                       /* of the proportional draw */
    /* the tree, caller-owned device memory, root-major */
    int32_t *num_nodes;                              /* [P] */
    int32_t *parent, *depth, *visits, *num_children, *first_child; /* [P, N] */
    int32_t *node_action;                            /* [P, N, 3] */
    double *prior, *value_sum, *value_max;           /* [P, N] */
    uint8_t *terminal;                               /* [P, N] */
    double *reward_lo, *reward_hi;                   /* [P] */
    /* the move */
    int32_t *move_slot;                              /* [P]   written by CHOOSE, read by REROOT */
    int32_t *move_action;                            /* [P, 3] */
    int32_t *child_visits;                           /* [P, C] */
    int32_t *child_actions;                          /* [P, C, 3] */
    double *root_value;                              /* [P] */
    int32_t *remap;                                  /* [P, N] written by REROOT */
    const uint8_t *reset;                            /* [P] or NULL, read by REROOT */
    uint32_t *errors_dev;                            /* optional */
    void *stream;
} pcbenv_puct_move_request;
int pcbenv_puct_move(const pcbenv *env, const pcbenv_puct_move_request *req);

#ifdef __cplusplus
}
#endif
#endif /* PCBENV_MOVE_H */
