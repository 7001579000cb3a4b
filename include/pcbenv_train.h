/* pcbenv_train.h -- losses on the device that go beyond include/pcbenv.h: pcbenv_evaluate_visits and its backward call,
 * the AlphaZero policy loss -- the cross entropy of a masked policy against the visit counts of a searched move -- and its
 * gradient with respect to the logits.  An addition next to pcbenv.h, pcbenv_search.h, pcbenv_priors.h and pcbenv_move.h,
 * which stay as they are: the ABI version is pcbenv.h's and is unchanged, libpcbenv.so exports the entry points below as
 * well, and pcbenv/_train_lib.py binds them.
 *
 * Streams.  As pcbenv_evaluate_logits: each call only enqueues one kernel on its request's stream.
 *
 * What it replaces: nothing in the reference, which has no search.  It is what reads the training targets of a self-play
 * move (pcbenv_puct_move CHOOSE: child_visits, child_actions): pcbenv/visit_targets.py:cross_entropy_torch -- the bits
 * unpacked, log(mask) added, log_softmax over every logit, the visits scattered into a dense target, autograd -- as one
 * launch each way.
 */
#ifndef PCBENV_TRAIN_H
#define PCBENV_TRAIN_H

#include "pcbenv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Both calls take one request: one kernel launch on req->stream each.  Enqueue only, no allocation, no synchronisation.
 * Not meant to be captured into a hipGraph.  Rows are independent and num_rows is arbitrary (a minibatch of stored moves).
 * The handle supplies geometry (kind, O, H, W), the device and pcbenv_last_error only: no bound buffers are needed and
 * nothing the library owns is read or written.
 * Inputs, with the layouts of pcbenv_evaluate_logits.  logits: [num_rows, A], A = O*H*W, float32 or bf16, in the flat
 * action order a = o*H*W + x*W + y.  mask_bits: [num_rows, 2, H, ceil(W/64)] in the layout of pcbenv_mask_bits; orientation
 * o reads plane o & 1, the square kind reads plane 0 only, bits of columns >= W are ignored.  An illegal logit is never
 * read.  visits: int32 [num_rows, C] and target_actions: int32 [num_rows, C, 3] (PCBENV_ACTION_TUPLE) or [num_rows, C]
 * (PCBENV_ACTION_FLAT), C = num_targets: exactly the tensors pcbenv_puct_move CHOOSE writes (child_visits,
 * child_actions), any leading extents flattened into num_rows.
 * Forward (pcbenv_evaluate_visits).  L, M, w_i, Z, p_i and the entropy are those pcbenv.h defines for
 * pcbenv_evaluate_logits.  Entry c of a row is valid if visits[c] > 0, its action is in range and its bit is set.  T is
 * the int64 sum of the valid visits and pi_c = (double)visits[c] / (double)T.
 * cross_entropy = log Z - sum over the valid entries of pi_c (l_c - M), which is -sum pi_c log p_c: formed in float64,
 * rounded once to float32.  Entries with the same action add up.  A valid entry whose logit is -inf makes the cross
 * entropy +inf: that is data.  entropy is as in pcbenv_evaluate_logits.  stats: float32 [num_rows, 4] = (M, log Z,
 * entropy, row status), 16-byte aligned, what the backward call reads; row status is 0 (ROW_OK), 1 (ROW_ZERO: the gradient
 * row is zero) or 2 (ROW_NO_TARGET: the row is a distribution but T == 0).  cross_entropy, entropy, stats (no gradient
 * wanted) and errors_dev may be NULL.  The gradient members of the request are not read.
 * Backward (pcbenv_evaluate_visits_backward).  Writes every element of grad_logits [num_rows, A] in the logits' dtype
 * (bf16: round to nearest even), each exactly once: the caller may pass uninitialised memory.
 *   g_i = g_ce (p_i - pi_i) - g_H p_i (log p_i + Hrow)   for i in L (pi_i = 0 off the targets; p_i = 0: the second term is 0)
 *   g_i = 0                                              for i not in L
 * with pi_i the sum of pi_c over the valid entries whose action is i (their visits summed as integers, divided by T once,
 * rounded to float32).  grad_cross_entropy (g_ce) and grad_entropy (g_H):
 * float32 [num_rows]; either may be NULL, which means zero.  stats is what the forward call wrote for the same rows;
 * cross_entropy, entropy and errors_dev are not touched.
 * Edge cases are data, never errors; the first line that applies to a row decides:
 *   no legal action:                   both outputs 0, gradient row zero, no bit
 *   a legal NaN or +inf:               bit 0 (value 1); cross_entropy = entropy = log n, n = |L|; gradient row zero
 *   every legal logit -inf:            bit 1 (value 2); the same outputs
 * and otherwise, entry by entry:
 *   visits[c] == 0:                    the entry is ignored, no bit (CHOOSE zero-fills behind k; unvisited children)
 *   visits[c] < 0, or > 0 with an action out of range or not legal:   the entry is ignored, bit 2 (value 4)
 *   T == 0:                            cross_entropy = 0, entropy as usual, the g_ce term dropped, ROW_NO_TARGET
 * The forward call ORs the bits into *errors_dev.
 * PCBENV_EINVAL (checked before any device call, in this order): null request; struct_size not
 * sizeof(pcbenv_visits_request); unknown logits_dtype; unknown action_format; num_targets outside
 * [1, PCBENV_MAX_TREE_CHILDREN]; num_rows < 0 or above INT32_MAX; reserved != 0; null logits, mask_bits, visits or
 * target_actions; (backward) null stats or grad_logits; logits not aligned to its element size; mask_bits not 8-byte
 * aligned; visits or target_actions not 4-byte aligned; stats not 16-byte aligned; (backward) grad_logits not aligned to
 * its element size; null handle.  num_rows == 0 is a no-op success. */
typedef struct pcbenv_visits_request {
    uint32_t struct_size; int32_t logits_dtype;      /* PCBENV_LOGITS_F32 / PCBENV_LOGITS_BF16 */
    int32_t action_format, num_targets /*C*/;        /* PCBENV_ACTION_TUPLE / PCBENV_ACTION_FLAT */
    int64_t num_rows, reserved /*0*/;
    const void *logits;                              /* [num_rows, A], flat action order */
    const uint64_t *mask_bits;                       /* [num_rows, 2, H, ceil(W/64)] */
    const int32_t *visits;                           /* [num_rows, C] */
    const int32_t *target_actions;                   /* [num_rows, C, 3] / [num_rows, C] */
    float *cross_entropy;                            /* [num_rows], forward, optional */
    float *entropy;                                  /* [num_rows], forward, optional */
    float *stats;                                    /* [num_rows, 4]: written by forward (optional), read by backward */
    uint32_t *errors_dev;                            /* forward, optional */
    const float *grad_cross_entropy;                 /* [num_rows], backward, optional */
    const float *grad_entropy;                       /* [num_rows], backward, optional */
    void *grad_logits;                               /* [num_rows, A] in the logits' dtype, backward */
    void *stream;
} pcbenv_visits_request;
int pcbenv_evaluate_visits(const pcbenv *env, const pcbenv_visits_request *req);
int pcbenv_evaluate_visits_backward(const pcbenv *env, const pcbenv_visits_request *req);

#ifdef __cplusplus
}
#endif
#endif /* PCBENV_TRAIN_H */
