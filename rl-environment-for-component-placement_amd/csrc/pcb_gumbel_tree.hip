// pcb_gumbel_tree.hip -- k_gumbel_tree and its entry point pcbenv_gumbel_tree_advance (include/pcbenv_gumbel_tree.h): the
// tree step of a batch of searches under the full Gumbel rule -- Sequential Halving at the root, argmax (pi' - N / (1 + sum
// N)) at every other level, v_mix as the value of a child without a visit at every node -- on the device (what
// pcbenv/search.py:gumbel_node_scores and gumbel_select_node do per level with a chain of gathers, a loop of masked sums, an
// ln and an exp per child over [P, C]).  Part of libpcbenv.so (CDNA4 / gfx950 only); a translation unit of its own, host side
// included, so that nothing here can change the builds of the other kernels or of the other entry points.
//
// The rule of one node is pcb_gumbel_tree.h (tree_select, tree_choose: the text tools/gumbel_tree_check.cpp runs on the CPU)
// over pcb_gumbel.h; the kernel composes the same pieces on pcb_group.h's mapping: G = group_lanes(C) lanes per root, lane c at
// child c of the current node, 256 / G roots per workgroup.  Groups share nothing: no LDS, no barrier.
//   a level          two load round trips, PCB_PUCT_DESCEND's: the node's terminal, num_children, first_child, visits and
//                    value_sum together, then the children's visits, value_sum and prior -- consecutive slots.  Lane c then
//                    holds n_c, value_sum(ch), pr_c and pr_c * q_c of its child.  max n_b and the largest improved logit are
//                    shuffle butterflies of a maximum, Nsum one of a 64-bit integer sum: order-free operations.  S, Wv and
//                    Qv are formed by every lane of the group in ONE loop over lane shuffles of the three addends, child
//                    after child, the visited children named by one ballot; Z, which depends on vmix and so on the first
//                    loop, in a second one.  The order of the sums is the contract, so there is no tree reduction, and all
//                    lanes hold the same bits.  One ln and one exp per lane and level; the argmax is pcb_group.h's.
//   the root level   in a scheduled simulation lane c adds g_c (two more ln) and the group takes k_gumbel_advance's argmax over
//                    the children at the considered count.
//   choose           k_gumbel_advance's, with the level's quantities at node 0.
//   absorb           k_puct_advance's absorb: pcb_puct_group.h's absorb_phase, over this unit's argument block.
#include <hip/hip_runtime.h>

#include "pcb_group.h"
#include "pcb_tree_host.h"
#include "pcbenv_gumbel_tree.h"
#include "pcb_gumbel_tree.h"
#include "pcb_puct_group.h"

static_assert(PCBENV_GUMBEL_BEGIN == pcb_gumbel::PHASE_BEGIN && PCBENV_GUMBEL_ABSORB == pcb_gumbel::PHASE_ABSORB &&
              PCBENV_GUMBEL_SELECT == pcb_gumbel::PHASE_SELECT && PCBENV_GUMBEL_CHOOSE == pcb_gumbel::PHASE_CHOOSE &&
              PCBENV_MAX_TREE_CHILDREN == pcb_gumbel::MAX_CHILDREN, "pcbenv_gumbel.h and pcb_gumbel.h name the same phases and bound");
static_assert(sizeof(pcbenv_gumbel_request) == 344, "pcbenv/_gumbel_lib.py:PcbenvGumbelRequest");

namespace {

using namespace pcb_gumbel_tree;
using namespace pcb_puct;
using pcb_group::BLOCK;
using pcb_group::fence;
using pcb_group::group_ballot;

// what the kernel needs of a request: c_puct is not among it
struct GumbelTreeArgs {
    int phases, P, N, C, T, K;
    Rule q;
    int *num_nodes, *parent, *depth, *visits, *num_children, *first_child, *node_action;
    double *prior, *value_sum, *value_max;
    uint8_t *terminal;
    double *lo, *hi;
    int *selected, *path_len, *paths;
    const double *value;
    const uint8_t *leaf_terminal;
    const int *cand_count, *cand_actions;
    const float *cand_prior;
    int *sim_index, *sim_visits;
    const int *considered;
    int *move_slot, *move_action, *child_weights;
    float *child_policy;
    int *child_actions;
    double *root_value;
    unsigned *errors;
};

// the largest of v over the G lanes of a group (every lane ends with it): a shuffle butterfly
template <int G, class V> __device__ inline V group_max(V v) {
    #pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v = larger(v, __shfl_xor(v, o));
    return v;
}
// the sum of v over the G lanes of a group: integers, so the order is free
template <int G> __device__ inline long long group_sum(long long v) {
    #pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// v of lane b of this lane's group, b the same in every lane.  A group of 64 is the wavefront, so b names one lane for all of
// it and the value comes by two scalar lane reads; a narrower group reads its own lane b through the cross-lane network
template <int G> __device__ inline double lane_value(double v, int b) {
    if constexpr (G == 64) {
        const long long u = __double_as_longlong(v);
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)u, b), hi = (unsigned)__builtin_amdgcn_readlane((int)(u >> 32), b);
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    } else return __shfl(v, b, G);
}

// what lane c holds of child fc + c of a node: its logit, its sigma, its visits, and the visits of all the children
struct Child { double lg, sg; int n; long long Nsum; };
// node_logits: k and fc have passed children_ok, vis and sum are the node's; a lane without a child holds numbers nobody reads
template <int G> __device__ inline Child node_child_of_lane(const Root &r, const GumbelTreeArgs &a, int lane, int base, int k, int fc, int vis, double sum,
                                                            double lo, double hi) {
    const bool mine = lane < k;
    const int ch = fc + (mine ? lane : 0);
    const int n_c = r.visits[ch];
    const double vs = r.value_sum[ch], prior = r.prior[ch];
    const bool seen = mine && n_c > 0;
    const double pr = clamped_prior(prior), q_c = vs / (double)(seen ? n_c : 1), wq = pr * q_c;
    const int most = group_max<G>(mine ? n_c : INT_MIN);
    const long long Nsum = group_sum<G>(mine ? (long long)n_c : 0ll);
    const unsigned long long seen_by = group_ballot<G>(seen, base);
    double S = 0.0, Wv = 0.0, Qv = 0.0;
    #pragma unroll 4
    for (int b = 0; b < G; b++) {  // in this order: it is the contract
        const double vb = lane_value<G>(vs, b), wb = lane_value<G>(pr, b), qb = lane_value<G>(wq, b);
        const bool on = (seen_by >> b) & 1ull;
        S = b < k ? S + vb : S;
        Wv = on ? Wv + wb : Wv;
        Qv = on ? Qv + qb : Qv;
    }
    const double vmix = mixed_value(own_value(sum, vis, S, Nsum, lo), Nsum, Wv, Qv);
    return Child{ieee_ln(pr), sigma(completed(seen ? q_c : vmix, lo, hi), most, a.q.c_visit, a.q.c_scale), n_c, Nsum};
}
// node_policy: pi of this lane's child, 0 for a lane without one
template <int G> __device__ inline double policy_of_lane(double x, bool mine, int k) {
    const double mx = group_max<G>(mine ? x : neg_inf());
    const double e = mine ? ieee_exp(x - mx) : 0.0;
    double Z = 0.0;
    #pragma unroll 4
    for (int b = 0; b < G; b++) {  // in this order: it is the contract
        const double eb = lane_value<G>(e, b);
        Z = b < k ? Z + eb : Z;
    }
    return e / Z;
}

template <int G> __device__ inline void begin_phase(const Root &r, const GumbelTreeArgs &a, int lane) {
    if (lane == 0) a.sim_index[r.p] = 0;
    if (lane < r.C) a.sim_visits[(long long)r.p * r.C + lane] = 0;
}

// tree_select: the root level by the schedule, then tree_descend's levels, child first_child + c of the current node in lane c
template <int G> __device__ inline unsigned select_phase(const Root &r, const GumbelTreeArgs &a, int lane, int base) {
    unsigned err = 0u;
    const double lo = *r.lo, hi = *r.hi;
    int node = 0, d = 0;
    const int term0 = r.terminal[0], k0 = r.num_children[0], fc0 = r.first_child[0], vis0 = r.visits[0];
    const double sum0 = r.value_sum[0];
    bool go = !stops(term0, k0);
    if (go) {
        const int t = a.sim_index[r.p];
        if (!children_ok(fc0, k0, r.N, r.C) || t < 0) { err |= ERR_TREE; go = false; }
        else if (scheduled(t, a.q.n)) {
            const bool mine = lane < k0;
            const int sim = mine ? a.sim_visits[(long long)r.p * r.C + lane] : 0;
            const Child me = node_child_of_lane<G>(r, a, lane, base, k0, fc0, vis0, sum0, lo, hi);
            const double g = gumbel(draw_base(a.q.seed, a.q.first_root + r.p, a.q.step_index), lane);
            const int v = a.considered[(long long)considered_candidates(a.q.Mc, k0) * a.q.n + t];
            const bool at = mine && sim == v;
            const bool in = mine && (group_ballot<G>(at, base) == 0ull || at);
            double s = score(g, me.lg, me.sg);
            PCB_GROUP_ARGMAX(G, in, lane, s, c, beats)
            c = __shfl(c, base);  // lane 0's verdict
            node = fc0 + c;
            if (lane == c) a.sim_visits[(long long)r.p * r.C + lane] = one_more(sim);
            if (lane == 0) a.sim_index[r.p] = t + 1;
            if (lane < 3) a.paths[step_major(0, r.P, r.p, lane)] = r.node_action[3 * node + lane];
            d = 1;
        }
    }
    if (go) {
        for (; d < r.T; d++) {
            const int term = r.terminal[node], k = r.num_children[node], fc = r.first_child[node], vis = r.visits[node];
            const double sum = r.value_sum[node];
            if (stops(term, k)) break;
            if (!children_ok(fc, k, r.N, r.C)) { err |= ERR_TREE; break; }
            const bool mine = lane < k;
            const Child me = node_child_of_lane<G>(r, a, lane, base, k, fc, vis, sum, lo, hi);
            const double pi = policy_of_lane<G>(improved(me.lg, me.sg), mine, k);
            double s = mine ? excess(pi, me.n, me.Nsum) : neg_inf();
            PCB_GROUP_ARGMAX(G, mine, lane, s, c, beats)
            node = fc + __shfl(c, base);  // lane 0's verdict: one node per group whatever the scores were
            if (lane < 3) a.paths[step_major(d, r.P, r.p, lane)] = r.node_action[3 * node + lane];
        }
    }
    if (lane == 0) { a.selected[r.p] = node; a.path_len[r.p] = d; }
    return err;
}

// tree_choose, child first_child(0) + c in lane c
template <int G> __device__ inline unsigned choose_phase(const Root &r, const GumbelTreeArgs &a, int lane, int base) {
    unsigned err = 0u;
    int k = r.num_children[0];
    const int fc = r.first_child[0], visits0 = r.visits[0];
    const double sum0 = r.value_sum[0], lo = *r.lo, hi = *r.hi;
    if (k != 0 && !children_ok(fc, k, r.N, r.C)) { err |= ERR_TREE; k = 0; }
    const bool mine = lane < k;
    int act[3] = {0, 0, 0};
    double pi = 0.0;
    int c = 0;
    if (k > 0) {  // the whole group
        const int sim = mine ? a.sim_visits[(long long)r.p * r.C + lane] : 0;
        const Child me = node_child_of_lane<G>(r, a, lane, base, k, fc, visits0, sum0, lo, hi);
        const double g = gumbel(draw_base(a.q.seed, a.q.first_root + r.p, a.q.step_index), lane);
        const int ch = fc + (mine ? lane : 0);
        #pragma unroll
        for (int i = 0; i < 3; i++) act[i] = mine ? r.node_action[3 * ch + i] : 0;
        const int most = group_max<G>(mine ? sim : INT_MIN);
        pi = policy_of_lane<G>(improved(me.lg, me.sg), mine, k);
        const bool in = mine && sim == most;
        double s = score(g, me.lg, me.sg);
        PCB_GROUP_ARGMAX(G, in, lane, s, best, beats)
        c = __shfl(best, base);
    }
    if (lane < r.C) {
        const long long row = (long long)r.p * r.C + lane;
        a.child_weights[row] = mine ? weight(pi) : 0;
        a.child_policy[row] = mine ? (float)pi : 0.0f;
        #pragma unroll
        for (int i = 0; i < 3; i++) a.child_actions[3 * row + i] = act[i];
    }
    #pragma unroll
    for (int i = 0; i < 3; i++) act[i] = __shfl(act[i], base + c);  // zeros without children
    if (lane == 0) {
        a.move_slot[r.p] = k > 0 ? fc + c : -1;
        a.root_value[r.p] = pcb_move::mean_value(sum0, visits0);
    }
    if (lane < 3) a.move_action[3 * (long long)r.p + lane] = lane == 0 ? act[0] : lane == 1 ? act[1] : act[2];
    return err;
}

template <int G> __global__ __launch_bounds__(BLOCK) void k_gumbel_tree(const GumbelTreeArgs a) {
    PCB_GROUP_ENTER(G, a);
    const Root r = root_of_group(a, (int)p, a.T);
    unsigned err = 0u;
    if (a.phases & pcb_gumbel::PHASE_BEGIN) {
        begin_phase<G>(r, a, lane);
        fence();
    }
    if (a.phases & pcb_gumbel::PHASE_ABSORB) {
        err |= absorb_phase<G>(r, a, lane, base);
        fence();
    }
    if (a.phases & pcb_gumbel::PHASE_SELECT) err |= select_phase<G>(r, a, lane, base);
    if (a.phases & pcb_gumbel::PHASE_CHOOSE) err |= choose_phase<G>(r, a, lane, base);
    if (err != 0u && lane == 0 && a.errors) atomicOr(a.errors, err);
}

bool finite_not_negative(double x) { return x >= 0.0 && x <= 1.7976931348623157e308; }

}  // namespace

// ---- pcbenv_gumbel_tree_advance ----------------------------------------------------------------------------------
// pcbenv_gumbel_advance's checks, in its order: every argument check before a device is touched, the null handle last; then
// one launch.
extern "C" int pcbenv_gumbel_tree_advance(const pcbenv *cenv, const pcbenv_gumbel_request *q) {
    using namespace pcb_tree_host;
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    PCB_TRY(check_request(env, q, "pcbenv_gumbel_request"));
    const int ph = q->phases;
    const bool begin = ph & PCBENV_GUMBEL_BEGIN, choose = ph & PCBENV_GUMBEL_CHOOSE;
    const Phases tree{false, (ph & PCBENV_GUMBEL_ABSORB) != 0, (ph & PCBENV_GUMBEL_SELECT) != 0};
    if (ph == 0 || (ph & ~(PCBENV_GUMBEL_BEGIN | PCBENV_GUMBEL_ABSORB | PCBENV_GUMBEL_SELECT | PCBENV_GUMBEL_CHOOSE)) != 0)
        return fail(env, PCBENV_EINVAL, "phases must be a non-empty set of BEGIN, ABSORB, SELECT, CHOOSE");
    if (choose && tree.select) return fail(env, PCBENV_EINVAL, "phases: CHOOSE cannot be combined with SELECT");
    PCB_TRY(check_extents(env, q));
    if (q->max_steps < 1) return fail(env, PCBENV_EINVAL, "max_steps must be at least 1");
    PCB_TRY(check_puct_candidates(env, q, tree));
    if (q->num_simulations < 1) return fail(env, PCBENV_EINVAL, "num_simulations must be at least 1");
    if (q->max_considered < 1 || q->max_considered > MAX_CONSIDERED) return fail(env, PCBENV_EINVAL, "max_considered must be in [1, 64]");
    if (q->reserved != 0) return fail(env, PCBENV_EINVAL, "reserved must be 0");
    if (!finite_not_negative(q->c_visit) || !finite_not_negative(q->c_scale)) return fail(env, PCBENV_EINVAL, "c_visit and c_scale must be finite and not negative");
    PCB_TRY(check_puct_tree(env, q));
    if ((begin || tree.select || choose) && (!q->sim_index || !q->sim_visits)) return fail(env, PCBENV_EINVAL, "null sim_index or sim_visits with BEGIN, SELECT or CHOOSE");
    if ((tree.absorb || tree.select) && !q->selected) return fail(env, PCBENV_EINVAL, "null selected");
    if (tree.select && (!q->path_len || !q->paths || !q->considered)) return fail(env, PCBENV_EINVAL, "null path_len, paths or considered with SELECT");
    PCB_TRY(check_puct_inputs(env, q, tree));
    if (choose && (!q->move_slot || !q->move_action || !q->child_weights || !q->child_policy || !q->child_actions || !q->root_value))
        return fail(env, PCBENV_EINVAL, "null move_slot, move_action, child_weights, child_policy, child_actions or root_value with CHOOSE");
    PCB_TRY(check_puct_doubles(env, q, tree.absorb ? q->value : 0));
    if (choose && ((uintptr_t)q->root_value & 7u) != 0) return fail(env, PCBENV_EINVAL, "the float64 tensors must be 8-byte aligned");
    PCB_TRY(check_cand_prior(env, q, tree));
    if (choose && ((uintptr_t)q->child_policy & 3u) != 0) return fail(env, PCBENV_EINVAL, "child_policy must be 4-byte aligned");
    PCB_TREE_CHECKS_END(env, q);
    GumbelTreeArgs a;
    puct_tree_args(a, q);
    a.T = q->max_steps; a.K = q->num_candidates;
    a.selected = q->selected; a.path_len = q->path_len; a.paths = q->paths; a.value = q->value; a.leaf_terminal = q->leaf_terminal;
    a.cand_count = q->cand_count; a.cand_actions = q->cand_actions; a.cand_prior = q->cand_prior;
    a.q = Rule{0.0, q->c_visit, q->c_scale, q->seed, q->step_index, q->first_root, q->num_simulations, q->max_considered};
    a.sim_index = q->sim_index; a.sim_visits = q->sim_visits; a.considered = q->considered;
    a.move_slot = q->move_slot; a.move_action = q->move_action; a.child_weights = q->child_weights; a.child_policy = q->child_policy;
    a.child_actions = q->child_actions; a.root_value = q->root_value;
    PCB_GROUP_LAUNCH(k_gumbel_tree, a, (hipStream_t)q->stream);
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}
