// pcb_tree_host.h -- the argument checks the tree entry points share (pcbenv_tree_advance, pcbenv_puct_advance,
// pcbenv_puct_advance_leaves, pcbenv_puct_move), stated once, and the copy of a request's PUCT tree into a kernel's
// argument block.  Host side of libpcbenv.so.  An entry point is a list: these pieces in the order its ABI test pins,
// its own checks between them, then the launch -- every check before a device is touched, the null handle last.
//
// A check is a function template over the request type (the requests name their common members alike); it records the
// message through fail() and returns its code, PCBENV_OK if there is nothing to say.  PCB_TRY returns the first failure.
#pragma once
#include "pcb_host.h"

#define PCB_TRY(check) do { const int rc_ = (check); if (rc_ != PCBENV_OK) return rc_; } while (0)

namespace pcb_tree_host {

// the head of every request: it exists and is the struct this library was built with
template <class Q> int check_request(pcbenv *env, const Q *q, const char *type) {
    if (!q) return fail(env, PCBENV_EINVAL, "null request");
    if (q->struct_size != (uint32_t)sizeof(Q)) return fail(env, PCBENV_EINVAL, "struct_size is not sizeof(%s)", type);
    return PCBENV_OK;
}
// phases of a tree step: a set of PCBENV_TREE_INIT, ABSORB, SELECT
struct Phases { bool init, absorb, select; };
inline Phases phases_of(int ph) { return Phases{(ph & PCBENV_TREE_INIT) != 0, (ph & PCBENV_TREE_ABSORB) != 0, (ph & PCBENV_TREE_SELECT) != 0}; }
inline int check_phases(pcbenv *env, int ph) {
    if (ph == 0 || (ph & ~(PCBENV_TREE_INIT | PCBENV_TREE_ABSORB | PCBENV_TREE_SELECT)) != 0) return fail(env, PCBENV_EINVAL, "phases must be a non-empty set of INIT, ABSORB, SELECT");
    if ((ph & PCBENV_TREE_INIT) && (ph & PCBENV_TREE_ABSORB)) return fail(env, PCBENV_EINVAL, "phases: INIT cannot be combined with ABSORB");
    return PCBENV_OK;
}
// the extents of every tree: P roots, N slots, C children
template <class Q> int check_extents(pcbenv *env, const Q *q) {
    if (q->num_roots < 0) return fail(env, PCBENV_EINVAL, "num_roots must not be negative");
    if (q->capacity < 1) return fail(env, PCBENV_EINVAL, "capacity must be at least 1");
    if (q->max_children < 1 || q->max_children > PCBENV_MAX_TREE_CHILDREN) return fail(env, PCBENV_EINVAL, "max_children must be in [1, 64]");
    return PCBENV_OK;
}
// the head of a search request: the struct, its phases, the extents and T steps
template <class Q> int check_search_request(pcbenv *env, const Q *q, const char *type) {
    PCB_TRY(check_request(env, q, type));
    PCB_TRY(check_phases(env, q->phases));
    PCB_TRY(check_extents(env, q));
    return q->max_steps < 1 ? fail(env, PCBENV_EINVAL, "max_steps must be at least 1") : PCBENV_OK;
}
// what SELECT writes and ABSORB reads back
template <class Q> int check_exchange(pcbenv *env, const Q *q, Phases ph) {
    if ((ph.absorb || ph.select) && !q->selected) return fail(env, PCBENV_EINVAL, "null selected");
    if (ph.select && (!q->path_len || !q->paths)) return fail(env, PCBENV_EINVAL, "null path_len or paths with SELECT");
    return PCBENV_OK;
}

// ---- the PUCT tree (include/pcbenv_search.h) and the evaluation ABSORB takes --------------------------------------------
// `more_null`: a tree tensor of the caller's own (pending) is null
template <class Q> int check_puct_tree(pcbenv *env, const Q *q, bool more_null = false) {
    if (!q->num_nodes || !q->parent || !q->depth || !q->visits || !q->num_children || !q->first_child || !q->node_action || !q->prior ||
        !q->value_sum || !q->value_max || !q->terminal || !q->reward_lo || !q->reward_hi || more_null) return fail(env, PCBENV_EINVAL, "null tree tensor");
    return PCBENV_OK;
}
template <class Q> int check_puct_candidates(pcbenv *env, const Q *q, Phases ph) {
    return ph.absorb && q->num_candidates < 1 ? fail(env, PCBENV_EINVAL, "num_candidates must be at least 1 with ABSORB") : PCBENV_OK;
}
template <class Q> int check_puct_inputs(pcbenv *env, const Q *q, Phases ph) {
    if (ph.absorb && (!q->value || !q->leaf_terminal || !q->cand_count || !q->cand_actions || !q->cand_prior))
        return fail(env, PCBENV_EINVAL, "null value, leaf_terminal, cand_count, cand_actions or cand_prior with ABSORB");
    return PCBENV_OK;
}
// `also`: the float64 tensor of the phase that runs, null otherwise
template <class Q> int check_puct_doubles(pcbenv *env, const Q *q, const double *also) {
    const uintptr_t doubles = (uintptr_t)q->prior | (uintptr_t)q->value_sum | (uintptr_t)q->value_max | (uintptr_t)q->reward_lo |
                              (uintptr_t)q->reward_hi | (uintptr_t)also;
    return (doubles & 7u) != 0 ? fail(env, PCBENV_EINVAL, "the float64 tensors must be 8-byte aligned") : PCBENV_OK;
}
template <class Q> int check_cand_prior(pcbenv *env, const Q *q, Phases ph) {
    return ph.absorb && ((uintptr_t)q->cand_prior & 3u) != 0 ? fail(env, PCBENV_EINVAL, "cand_prior must be 4-byte aligned") : PCBENV_OK;
}

// the extents and the tree tensors of a request into the members of the same meaning of k_puct_advance's, k_puct_leaves'
// and k_puct_move's argument blocks
template <class A, class Q> void puct_tree_args(A &a, const Q *q) {
    a.phases = q->phases; a.P = q->num_roots; a.N = q->capacity; a.C = q->max_children;
    a.num_nodes = q->num_nodes; a.parent = q->parent; a.depth = q->depth; a.visits = q->visits; a.num_children = q->num_children;
    a.first_child = q->first_child; a.node_action = q->node_action; a.prior = q->prior; a.value_sum = q->value_sum; a.value_max = q->value_max;
    a.terminal = q->terminal; a.lo = q->reward_lo; a.hi = q->reward_hi; a.errors = (unsigned *)q->errors_dev;
}
// and what a search exchanges with its caller
template <class A, class Q> void puct_search_args(A &a, const Q *q) {
    puct_tree_args(a, q);
    a.T = q->max_steps; a.K = q->num_candidates; a.c_puct = q->c_puct;
    a.selected = q->selected; a.path_len = q->path_len; a.paths = q->paths; a.value = q->value; a.leaf_terminal = q->leaf_terminal;
    a.cand_count = q->cand_count; a.cand_actions = q->cand_actions; a.cand_prior = q->cand_prior;
}

}  // namespace pcb_tree_host

// ---- the tail of the checks: the handle, nothing to do, the handle's device for the rest of the function -----------------
#define PCB_TREE_CHECKS_END(env, q) \
    if (!env) return fail(0, PCBENV_EINVAL, "null handle"); \
    if (q->num_roots == 0) return PCBENV_OK; \
    DEVICE_GUARD(env)
