/* pcbenv_noise.h -- exploration noise for a searched game on the device, beyond include/pcbenv.h: pcbenv_puct_root_noise,
 * which mixes a draw from Dir(alpha) into the priors of the children of every root of a PUCT tree, once per move.  An
 * addition next to pcbenv.h, pcbenv_search.h, pcbenv_priors.h, pcbenv_move.h, pcbenv_train.h and pcbenv_leaves.h, which
 * stay as they are: the ABI version is pcbenv.h's and is unchanged, libpcbenv.so exports the entry point below as well,
 * and pcbenv/_noise_lib.py binds it.
 *
 * Streams.  As pcbenv_puct_move: the call only enqueues one kernel on its request's stream.
 *
 * What it replaces: nothing in the reference, which has no search.  It is the P(s, a) = (1 - eps) p_a + eps eta_a of
 * AlphaZero's self-play at the root, where the priors live: in the tree, on the device.  pcbenv/search.py:puct_root_noise
 * is the specification, which the kernel matches bit for bit.
 */
#ifndef PCBENV_NOISE_H
#define PCBENV_NOISE_H

#include "pcbenv_search.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Dirichlet noise on the root priors of P PUCT trees (the tree tensors of pcbenv_puct_request it names, same names, dtypes
 * and layouts), one kernel launch on req->stream.  The caller owns every tensor; the handle supplies the device and
 * pcbenv_last_error only: nothing the library owns is read or written and no bound buffers are needed.  Enqueue only, no
 * allocation, no synchronisation, one kernel on req->stream.  Not meant to be captured into a hipGraph.
 * N = capacity node slots per root, C = max_children.
 * Which roots.  Let k = num_children(0) and fc = first_child(0).  Root p is handled only if noised[p] == 0 and k >= 1.
 * Both are then checked (k <= C, 1 <= fc <= N - k) before they address anything; a root that fails is left untouched,
 * ORs bit 1 (value 2) into *errors_dev and keeps noised[p] = 0.  A handled root gets noised[p] = 1.  A root without
 * children is left alone with noised[p] = 0, so that a later call finds it.  The caller zeroes noised when the search of a
 * move begins; a second call on the same tensors is a no-op.  Nothing but prior of the k children and noised[p] is ever
 * stored.
 * The uniform stream.  base = mix64(mix64(seed ^ 0x9E3779B97F4A7C15 * (first_root + p + 1)) + step_index), the 64 bits
 * behind the draw of pcbenv_sample_actions; draw number t of child c is w = mix64(base + 0x9E3779B97F4A7C15 * (64 t + c +
 * 1)) and u = ((w >> 12) + 0.5) * 2^-52, exact in a double and strictly inside (0, 1).  A value depends on (seed, first_root
 * + p, step_index, c, t) alone: never on P, on C or on the other children.
 * Gamma(alpha) for child c (Marsaglia and Tsang, a bounded loop).  a = alpha if alpha >= 1, else alpha + 1; d = a - 1/3;
 * cc = (1/3) / sqrt(d).  Attempt t = 0 .. 31 takes draws 3 t, 3 t + 1, 3 t + 2: v1 = 2 u1 - 1, v2 = 2 u2 - 1, s = v1 v1 +
 * v2 v2, the attempt fails if s >= 1; x = v1 * sqrt((-2 ln s) / s), v = (1 + cc x)^3, the attempt fails if v <= 0; it is
 * accepted if ln u3 < ((0.5 (x x) + d) - d v) + d ln v, and then g = d v.  If all 32 attempts fail, g = d.  alpha < 1:
 * g = g * exp(ln(u) / alpha) with draw number 96.  ln, exp and sqrt are the library's own, written in IEEE + - * / alone
 * (csrc/pcb_ieee_math.h), one IEEE operation per written operator: relative error below 5e-16, the same bits everywhere.
 * The mix.  S = g_0 + g_1 + ... + g_(k-1), summed in that order; eta_c = g_c / S, or 1 / k if S is not a finite number
 * greater than 0; prior(fc + c) = (double)(float)((1 - eps) * prior(fc + c) + eps * eta_c), 1 - eps formed once.  A noised
 * prior is a float32 value, as every prior an evaluator gives is: with eps = 0 a tree of float32 priors is unchanged bit
 * for bit.
 * Layouts: num_children, first_child int32 [P, N]; prior float64 [P, N]; noised int32 [P]; errors_dev may be NULL.
 * PCBENV_EINVAL (checked before any device call, in this order): null request; struct_size not
 * sizeof(pcbenv_puct_noise_request); num_roots < 0; capacity < 1; max_children outside [1, PCBENV_MAX_TREE_CHILDREN];
 * reserved != 0; alpha not finite or outside [0.01, 100]; eps not finite or outside [0, 1]; a null tensor among
 * num_children, first_child, prior, noised; prior not 8-byte aligned; null handle.  num_roots == 0 is a no-op success. */
typedef struct pcbenv_puct_noise_request {
    uint32_t struct_size;
    int32_t num_roots /*P*/, capacity /*N node slots per root*/, max_children /*C*/, first_root /*global index of root 0 in the draw hash*/, reserved /*0*/;
    uint64_t seed, step_index;                       /* of the noise draws */
    double alpha, eps;
    /* of the tree, caller-owned device memory, root-major */
    int32_t *num_children, *first_child;             /* [P, N] */
    double *prior;                                   /* [P, N] */
    int32_t *noised;                                 /* [P] */
    uint32_t *errors_dev;                            /* optional */
    void *stream;
} pcbenv_puct_noise_request;
int pcbenv_puct_root_noise(const pcbenv *env, const pcbenv_puct_noise_request *req);

#ifdef __cplusplus
}
#endif
#endif /* PCBENV_NOISE_H */
