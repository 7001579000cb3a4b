/* pcbenv_priors.h -- policy priors on the device that go beyond include/pcbenv.h: pcbenv_top_priors, the K most probable
 * legal actions of a masked policy and their probabilities.  An addition next to pcbenv.h and pcbenv_search.h, which stay
 * as they are: the ABI version is pcbenv.h's and is unchanged, libpcbenv.so exports the entry point below as well, and
 * pcbenv/_priors_lib.py binds it.
 *
 * Streams.  As pcbenv_evaluate_logits: the call only enqueues one kernel on its request's stream.
 *
 * What it replaces: nothing in the reference, which has no search.  It is the step between a policy network and
 * pcbenv_puct_advance: pcbenv/search.py:top_priors as one launch, with the order of the candidates defined on the logits
 * instead of on their float32 probabilities.
 */
#ifndef PCBENV_PRIORS_H
#define PCBENV_PRIORS_H

#include "pcbenv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The K = num_candidates largest legal logits of every row, in a defined order, with their probabilities under the masked
 * categorical of the row: one kernel launch on req->stream.  Enqueue only, no allocation, no synchronisation.  Not meant
 * to be captured into a hipGraph.  The three outputs have exactly the layouts pcbenv_puct_request reads (cand_count,
 * cand_actions, cand_prior), so they go into pcbenv_puct_advance with no tensor operation in between.
 * logits: [num_rows, A], A = O*H*W, float32 or bf16, in the flat action order a = o*H*W + x*W + y.
 * The legal set L of row r.  mask_bits given: rows are arbitrary, as in pcbenv_evaluate_logits -- bit rows
 * [num_rows, 2, H, ceil(W/64)] in the layout of pcbenv_mask_bits; orientation o reads plane o & 1, the square kind reads
 * plane 0 only, bits of columns >= W are ignored.  The handle supplies geometry and device only: no bound buffers are
 * needed and nothing the library owns is read or written.  mask_bits == NULL: row e is environment e, num_rows must be the
 * handle's num_envs, and the legal set is read from the bit rows of the handle's current state set, exactly as
 * pcbenv_sample_logits reads them; no mask is copied.  A logit outside the legal set has no influence: it may be NaN or
 * an already-masked value.
 * Order.  Let v_i be the legal logit i widened exactly to float32.  Candidates are ordered by v descending, compared as
 * IEEE values, so -0.0 equals +0.0; ties go to the lower flat index.  Legal -inf logits therefore come last, in index
 * order.
 * Outputs.  With n = |L| and k = min(K, n): cand_count[r] = k; cand_actions[r, c] = (o, x, y) of the c-th action in that
 * order, c < k; cand_prior[r, c] = float32(exp(v - M) / Z), M = max over L and Z = sum over L of exp(v - M) as for
 * pcbenv_sample_logits, formed in float64 and rounded once.  The priors are not renormalised over the k kept.  A -inf
 * logit has prior 0.  Entries c >= k are action (0, 0, 0) and prior 0.  Every element of the three outputs is written:
 * the caller may pass uninitialised memory.  The result is a function of the inputs alone: two launches give the same
 * bits (no floating-point atomics, a fixed reduction order).
 * Edge cases are data, never errors.  No legal action: count 0.  A legal NaN or +inf ORs bit 0 (value 1) into
 * *errors_dev, every legal logit -inf bit 1 (value 2); in both cases the candidates of that row are the first k legal
 * actions in flat order, each with prior float32(1.0 / n) -- the uniform fallback of pcbenv_sample_logits and
 * pcbenv_evaluate_logits.  errors_dev may be NULL.
 * PCBENV_EINVAL (checked before any device call, in this order): null request; struct_size not
 * sizeof(pcbenv_top_priors_request); unknown logits_dtype; num_candidates outside [1, PCBENV_MAX_TREE_CHILDREN];
 * reserved != 0; num_rows < 0 or above INT32_MAX; null logits, cand_count, cand_actions or cand_prior; logits not aligned
 * to its element size; mask_bits not 8-byte aligned; cand_count, cand_actions or cand_prior not 4-byte aligned; null
 * handle; mask_bits == NULL with num_rows != the handle's num_envs.
 * PCBENV_ESTATE (mask_bits == NULL only): pcbenv_bind_buffers has not been called, or the stream is being captured -- a
 * captured launch would keep reading the state set that was current at capture time.  num_rows == 0 is a no-op success. */
typedef struct pcbenv_top_priors_request {
    uint32_t struct_size; int32_t logits_dtype;      /* PCBENV_LOGITS_F32 / PCBENV_LOGITS_BF16 */
    int32_t num_candidates /*K*/, reserved /*0*/;
    int64_t num_rows;
    const void *logits;                              /* [num_rows, A], flat action order */
    const uint64_t *mask_bits;                       /* [num_rows, 2, H, ceil(W/64)] or NULL: the handle's current state set */
    int32_t *cand_count;                             /* [num_rows] */
    int32_t *cand_actions;                           /* [num_rows, K, 3] */
    float *cand_prior;                               /* [num_rows, K] */
    uint32_t *errors_dev;                            /* optional */
    void *stream;
} pcbenv_top_priors_request;
int pcbenv_top_priors(const pcbenv *env, const pcbenv_top_priors_request *req);

#ifdef __cplusplus
}
#endif
#endif /* PCBENV_PRIORS_H */
