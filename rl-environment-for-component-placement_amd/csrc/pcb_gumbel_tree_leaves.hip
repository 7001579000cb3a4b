// pcb_gumbel_tree_leaves.hip -- k_gumbel_tree_leaves and its entry point pcbenv_gumbel_tree_advance_leaves
// (include/pcbenv_gumbel_tree_leaves.h): the tree step of a batch of searches under the full Gumbel rule -- Sequential Halving
// at the root, argmax (pi' - (N + pending) / (1 + sum (N + pending))) at every other level, v_mix as the value of a child
// without a visit at every node -- with L descents per root and launch and the backup of all L evaluations (what
// pcbenv/search.py:gumbel_search(node_rule="gumbel", leaves=L) does in tensor code).  Part of libpcbenv.so (CDNA4 / gfx950
// only); a translation unit of its own, host side included, so that nothing here can change the builds of k_gumbel_leaves,
// k_gumbel_tree or the other entry points: the pieces of pcb_gumbel_leaves.hip and pcb_gumbel_tree.hip are composed here again,
// over this unit's argument block, and none of them moved.
//
// The rule of one root is pcb_gumbel_tree_leaves.h (tree_leaves_select: the text tools/gumbel_tree_leaves_check.cpp runs on the
// CPU) over pcb_gumbel_tree.h and pcb_gumbel_leaves.h; the kernel composes the same pieces on pcb_group.h's mapping: G =
// group_lanes(C) lanes per root, lane c at child c of the current node, 256 / G roots per workgroup.  Groups share nothing:
// no LDS, no barrier.
//   the prologue     k_gumbel_leaves': the root's children, their scores (pcb_gumbel_tree.h's, v_mix at the root) and their
//                    pending in registers for all L leaves, the counters committed once behind the last leaf, the table
//                    entries of the launch loaded in one round trip, the fence between leaves.
//   per leaf, root   one ballot and pcb_group.h's argmax, lane 0's verdict; the winner's fields by shuffle.
//   a level          the children of the node: visits, value_sum, prior, pending, and what the next level needs of the
//                    winner (terminal, num_children, first_child, the action) -- consecutive slots, ONE load round trip,
//                    k_gumbel_leaves' way: the winner's fields, its visits and value_sum among them, come by shuffle, so
//                    the node itself is never loaded.  Then k_gumbel_tree's arithmetic: max n_b and the largest improved
//                    logit are shuffle butterflies of a maximum, Nsum and Msum of a 64-bit integer sum; S, Wv and Qv are
//                    formed by every lane in ONE loop over lane shuffles of the three addends, child after child, Z in a
//                    second one -- the order of the sums is the contract.  One ln and one exp per lane and level.
//   choose           k_gumbel_tree's, with the level's quantities at node 0; absorb is k_gumbel_leaves'.
// A leaf reads what the leaf before it stored through other lanes of the same wavefront: the same fence stands between
// leaves as between phases.
#include <hip/hip_runtime.h>

#include "pcb_group.h"
#include "pcb_tree_host.h"
#include "pcbenv_gumbel_tree_leaves.h"
#include "pcb_gumbel_tree_leaves.h"

static_assert(PCBENV_GUMBEL_BEGIN == pcb_gumbel::PHASE_BEGIN && PCBENV_GUMBEL_ABSORB == pcb_gumbel::PHASE_ABSORB &&
              PCBENV_GUMBEL_SELECT == pcb_gumbel::PHASE_SELECT && PCBENV_GUMBEL_CHOOSE == pcb_gumbel::PHASE_CHOOSE &&
              PCBENV_MAX_TREE_CHILDREN == pcb_gumbel::MAX_CHILDREN && PCBENV_MAX_PUCT_LEAVES == pcb_puct_leaves::MAX_LEAVES,
              "pcbenv_gumbel.h, pcbenv_leaves.h, pcb_gumbel.h and pcb_puct_leaves.h name the same phases and bounds");
static_assert(sizeof(pcbenv_gumbel_leaves_request) == 360, "pcbenv/_gumbel_leaves_lib.py:PcbenvGumbelLeavesRequest");

namespace {

using namespace pcb_gumbel_tree_leaves;
using namespace pcb_puct;
using pcb_puct_leaves::leaves_back_up;
using pcb_group::BLOCK;
using pcb_group::fence;
using pcb_group::group_ballot;

// what the kernel needs of a request: c_puct is not among it
struct GumbelTreeLeavesArgs {
    int phases, P, N, C, T, K, L;
    Rule q;
    int *num_nodes, *parent, *depth, *visits, *num_children, *first_child, *node_action;
    double *prior, *value_sum, *value_max;
    uint8_t *terminal;
    double *lo, *hi;
    int *pending;
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

// what lane c holds of child fc + c of a node: its logit and its sigma; what the rule counts -- visits and pending; and what
// the next level needs if the child wins -- value_sum, terminal, num_children, first_child, the action
struct Child { double lg, sg, vs; int n, pn, term, k, fc, a0, a1, a2; };
// pcb_gumbel_tree.h:node_logits: k and fc have passed children_ok, vis and sum are the node's; a lane without a child holds
// numbers nobody reads.  One round trip: every load below depends on ch alone.  PENDING: SELECT's; CHOOSE does not read pending
template <int G, bool PENDING> __device__ inline Child child_of_lane(const Root &r, const GumbelTreeLeavesArgs &a, const int *pending, int lane, int base, int k, int fc,
                                                       int vis, double sum, double lo, double hi) {
    const bool mine = lane < k;
    const int ch = fc + (mine ? lane : 0);
    const int n_c = r.visits[ch], pn_c = PENDING ? pending[ch] : 0, term_c = r.terminal[ch], k_c = r.num_children[ch], fc_c = r.first_child[ch];
    const int a0 = r.node_action[3 * ch], a1 = r.node_action[3 * ch + 1], a2 = r.node_action[3 * ch + 2];
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
    return Child{ieee_ln(pr), sigma(completed(seen ? q_c : vmix, lo, hi), most, a.q.c_visit, a.q.c_scale), vs, n_c, pn_c, term_c, k_c, fc_c, a0, a1, a2};
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

template <int G> __device__ inline void begin_phase(const Root &r, const GumbelTreeLeavesArgs &a, int lane) {
    if (lane == 0) a.sim_index[r.p] = 0;
    if (lane < r.C) a.sim_visits[(long long)r.p * r.C + lane] = 0;
}

// leaves_absorb, the new children of a leaf over the lanes; returns the error bits (the same in every lane)
template <int G> __device__ inline unsigned absorb_phase(const Root &r, const GumbelTreeLeavesArgs &a, int *pending, int lane, int base) {
    unsigned err = 0u;
    int count = *r.num_nodes;
    double lo = *r.lo, hi = *r.hi;
    const long long row0 = (long long)r.p * a.L;
    int next = a.selected[row0];
    for (int l = 0; l < a.L; l++) {
        const long long row = row0 + l;
        const int selected = next;
        if (l + 1 < a.L) next = a.selected[row + 1];
        if (selected == -1) continue;
        if (!slot_ok(selected, r.N) || count < 1 || count > r.N) { err |= ERR_TREE; break; }
        if (l > 0) fence();
        const int node = selected, depth = r.depth[node], nch = r.num_children[node], term = r.terminal[node];
        const int leaf_terminal = a.leaf_terminal[row], cand_count = a.cand_count[row];
        const double value = a.value[row];
        if (leaf_terminal != 0) {
            if (lane == 0) r.terminal[node] = 1;
        } else if (expands(leaf_terminal, nch, term)) {
            const int k = kept_candidates(cand_count, a.K, r.C);
            if (k > 0 && count + k <= r.N) {
                const long long cand = row * a.K;
                if (lane < k) make_child(r, node, count + lane, depth, a.cand_actions + 3 * (cand + lane), a.cand_prior[cand + lane]);
                if (lane == 0) link_children(r, node, count, k);
                count += k;
            } else if (k > 0) err |= ERR_FULL;
        }
        lo = value < lo ? value : lo;
        hi = value > hi ? value : hi;
        unsigned up = 0u;
        if (lane == 0) up = leaves_back_up(r, pending, node, value);
        up = __shfl(up, base);
        err |= up;
        if (up & ERR_TREE) break;
    }
    if (lane == 0) { *r.lo = lo; *r.hi = hi; }
    return err;
}

// tree_leaves_select, child first_child + c of the current node in lane c
template <int G> __device__ inline unsigned select_phase(const Root &r, const GumbelTreeLeavesArgs &a, int *pending, int lane, int base) {
    constexpr int E = MAX_LEAVES / G;  // table entries a lane can be asked for: ceil(L / G) of them are loaded
    unsigned err = 0u;
    const double lo = *r.lo, hi = *r.hi;
    const int rows = a.P * a.L, row0 = r.p * a.L, n = a.q.n;
    // the root as every descent finds it: SELECT changes nothing of it but pending, which goes up by one per leaf
    const int term0 = r.terminal[0], k0 = r.num_children[0], fc0 = r.first_child[0], vis0 = r.visits[0];
    const double sum0 = r.value_sum[0];
    int pend0 = pending[0];
    const int t0 = a.sim_index[r.p];
    const bool halts = stops(term0, k0);
    int l = 0;
    if (halts || !children_ok(fc0, k0, r.N, r.C) || t0 < 0) {  // no descent: the root itself, once
        if (!halts) err |= ERR_TREE;
        if (lane == 0) { pending[0] = pend_more(pend0); a.selected[row0] = 0; a.path_len[row0] = 0; }
        l = 1;
    } else {
        const bool mine0 = lane < k0;
        // the schedule of this launch, before anything depends on it
        int table[E];
        const long long table_row = (long long)considered_candidates(a.q.Mc, k0) * n;
        #pragma unroll
        for (int e = 0; e < E; e++) {
            const int j = e * G + lane;
            table[e] = (j < a.L && (long long)t0 + j < n) ? a.considered[table_row + t0 + j] : 0;
        }
        // child c of the root in lane c: what no leaf changes, and pending, which only this group changes
        const int sim0 = mine0 ? a.sim_visits[(long long)r.p * r.C + lane] : 0;
        const Child root = child_of_lane<G, true>(r, a, pending, lane, base, k0, fc0, vis0, sum0, lo, hi);
        const double score0 = score(gumbel(draw_base(a.q.seed, a.q.first_root + r.p, a.q.step_index), lane), root.lg, root.sg);
        int pend_r = root.pn, sim = sim0, t = t0;
        for (; l < a.L; l++) {
            if (l > 0) fence();
            const int row = row0 + l;
            const bool on_schedule = t < n;
            if (!on_schedule && l > 0) break;  // out of budget: no evaluator row for an unscheduled descent
            int node = 0, d = 0, term = term0, k = k0, fc = fc0, vis = vis0, pend = pend0, win0 = 0;
            double sum = sum0;
            if (on_schedule) {
                const int i = t - t0;  // the leaves before this one committed i simulations
                int mine_v = 0;
                #pragma unroll
                for (int e = 0; e < E; e++) mine_v = (i / G == e) ? table[e] : mine_v;
                const int v = __shfl(mine_v, base + (i & (G - 1)));
                const bool at = mine0 && sim == v;
                const bool in = mine0 && (group_ballot<G>(at, base) == 0ull || at);
                double s = score0;
                PCB_GROUP_ARGMAX(G, in, lane, s, c, beats)
                win0 = __shfl(c, base) & (G - 1);  // lane 0's verdict: one node per group whatever the scores were
                if (lane == 0) pending[0] = pend_more(pend0);
                if (lane == win0) {
                    a.paths[step_major(0, rows, row, 0)] = root.a0; a.paths[step_major(0, rows, row, 1)] = root.a1; a.paths[step_major(0, rows, row, 2)] = root.a2;
                }
                node = fc0 + win0;
                term = __shfl(root.term, base + win0); k = __shfl(root.k, base + win0); fc = __shfl(root.fc, base + win0);
                vis = __shfl(root.n, base + win0); sum = __shfl(root.vs, base + win0); pend = __shfl(pend_r, base + win0);
                d = 1;
            }
            for (;; d++) {
                if (d >= r.T || stops(term, k)) break;
                if (!children_ok(fc, k, r.N, r.C)) { err |= ERR_TREE; break; }
                const bool mine = lane < k;
                const Child me = child_of_lane<G, true>(r, a, pending, lane, base, k, fc, vis, sum, lo, hi);
                const double pi = policy_of_lane<G>(improved(me.lg, me.sg), mine, k);
                const long long Msum = group_sum<G>(mine ? with_pending(me.n, me.pn) : 0ll);
                double s = mine ? excess(pi, me.n, me.pn, Msum) : neg_inf();
                PCB_GROUP_ARGMAX(G, mine, lane, s, c, beats)
                const int win = __shfl(c, base) & (G - 1);  // lane 0's verdict
                if (lane == 0) pending[node] = pend_more(pend);
                if (lane == win) {
                    a.paths[step_major(d, rows, row, 0)] = me.a0; a.paths[step_major(d, rows, row, 1)] = me.a1; a.paths[step_major(d, rows, row, 2)] = me.a2;
                }
                node = fc + win;
                term = __shfl(me.term, base + win); k = __shfl(me.k, base + win); fc = __shfl(me.fc, base + win);
                vis = __shfl(me.n, base + win); sum = __shfl(me.vs, base + win); pend = __shfl(me.pn, base + win);
            }
            if (repeats(term, k, pend)) {  // it consumes no simulation: the counters stay as they were before this leaf
                unsigned up = 0u;
                if (lane == 0) up = undo_pending(r, pending, node, d);
                err |= __shfl(up, base);
                break;
            }
            if (lane == 0) { pending[node] = pend_more(pend); a.selected[row] = node; a.path_len[row] = d; }
            pend0 = pend_more(pend0);
            if (on_schedule) {
                if (lane == win0) { sim = pcb_gumbel::one_more(sim); pend_r = pend_more(pend_r); }  // the root child was left or reached: one pending visit
                t += 1;
            }
        }
        if (t != t0) {
            if (mine0 && sim != sim0) a.sim_visits[(long long)r.p * r.C + lane] = sim;
            if (lane == 0) a.sim_index[r.p] = t;
        }
    }
    for (int j = l + lane; j < a.L; j += G) { a.selected[row0 + j] = -1; a.path_len[row0 + j] = -1; }  // no leaf
    return err;
}

// tree_choose, child first_child(0) + c in lane c
template <int G> __device__ inline unsigned choose_phase(const Root &r, const GumbelTreeLeavesArgs &a, int lane, int base) {
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
        const Child me = child_of_lane<G, false>(r, a, nullptr, lane, base, k, fc, visits0, sum0, lo, hi);
        const double g = gumbel(draw_base(a.q.seed, a.q.first_root + r.p, a.q.step_index), lane);
        act[0] = mine ? me.a0 : 0; act[1] = mine ? me.a1 : 0; act[2] = mine ? me.a2 : 0;
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

template <int G> __global__ __launch_bounds__(BLOCK) void k_gumbel_tree_leaves(const GumbelTreeLeavesArgs a) {
    PCB_GROUP_ENTER(G, a);
    const Root r = root_of_group(a, (int)p, a.T);
    int *const pending = a.pending + (long long)p * a.N;
    unsigned err = 0u;
    if (a.phases & pcb_gumbel::PHASE_BEGIN) {
        begin_phase<G>(r, a, lane);
        fence();
    }
    if (a.phases & pcb_gumbel::PHASE_ABSORB) {
        err |= absorb_phase<G>(r, a, pending, lane, base);
        fence();
    }
    if (a.phases & pcb_gumbel::PHASE_SELECT) err |= select_phase<G>(r, a, pending, lane, base);
    if (a.phases & pcb_gumbel::PHASE_CHOOSE) err |= choose_phase<G>(r, a, lane, base);
    if (err != 0u && lane == 0 && a.errors) atomicOr(a.errors, err);
}

bool finite_not_negative(double x) { return x >= 0.0 && x <= 1.7976931348623157e308; }

}  // namespace

// ---- pcbenv_gumbel_tree_advance_leaves ---------------------------------------------------------------------------
// pcbenv_gumbel_advance_leaves' checks, in its order: every argument check before a device is touched, the null handle last;
// then one launch.
extern "C" int pcbenv_gumbel_tree_advance_leaves(const pcbenv *cenv, const pcbenv_gumbel_leaves_request *q) {
    using namespace pcb_tree_host;
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    PCB_TRY(check_request(env, q, "pcbenv_gumbel_leaves_request"));
    const int ph = q->phases;
    const bool begin = ph & PCBENV_GUMBEL_BEGIN, choose = ph & PCBENV_GUMBEL_CHOOSE;
    const Phases tree{false, (ph & PCBENV_GUMBEL_ABSORB) != 0, (ph & PCBENV_GUMBEL_SELECT) != 0};
    if (ph == 0 || (ph & ~(PCBENV_GUMBEL_BEGIN | PCBENV_GUMBEL_ABSORB | PCBENV_GUMBEL_SELECT | PCBENV_GUMBEL_CHOOSE)) != 0)
        return fail(env, PCBENV_EINVAL, "phases must be a non-empty set of BEGIN, ABSORB, SELECT, CHOOSE");
    if (choose && tree.select) return fail(env, PCBENV_EINVAL, "phases: CHOOSE cannot be combined with SELECT");
    PCB_TRY(check_extents(env, q));
    if (q->max_steps < 1) return fail(env, PCBENV_EINVAL, "max_steps must be at least 1");
    if (q->num_leaves < 1 || q->num_leaves > PCBENV_MAX_PUCT_LEAVES) return fail(env, PCBENV_EINVAL, "num_leaves must be in [1, 64]");
    if ((long long)q->num_roots * q->num_leaves > 0x7fffffffLL) return fail(env, PCBENV_EINVAL, "num_roots * num_leaves must not exceed 2^31 - 1");
    PCB_TRY(check_puct_candidates(env, q, tree));
    if (q->num_simulations < 1) return fail(env, PCBENV_EINVAL, "num_simulations must be at least 1");
    if (q->max_considered < 1 || q->max_considered > pcb_gumbel::MAX_CONSIDERED) return fail(env, PCBENV_EINVAL, "max_considered must be in [1, 64]");
    if (q->reserved != 0 || q->reserved2 != 0) return fail(env, PCBENV_EINVAL, "reserved and reserved2 must be 0");
    if (!finite_not_negative(q->c_visit) || !finite_not_negative(q->c_scale)) return fail(env, PCBENV_EINVAL, "c_visit and c_scale must be finite and not negative");
    PCB_TRY(check_puct_tree(env, q, !q->pending));
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
    GumbelTreeLeavesArgs a;
    puct_tree_args(a, q);
    a.T = q->max_steps; a.K = q->num_candidates; a.L = q->num_leaves; a.pending = q->pending;
    a.selected = q->selected; a.path_len = q->path_len; a.paths = q->paths; a.value = q->value; a.leaf_terminal = q->leaf_terminal;
    a.cand_count = q->cand_count; a.cand_actions = q->cand_actions; a.cand_prior = q->cand_prior;
    a.q = Rule{0.0, q->c_visit, q->c_scale, q->seed, q->step_index, q->first_root, q->num_simulations, q->max_considered};
    a.sim_index = q->sim_index; a.sim_visits = q->sim_visits; a.considered = q->considered;
    a.move_slot = q->move_slot; a.move_action = q->move_action; a.child_weights = q->child_weights; a.child_policy = q->child_policy;
    a.child_actions = q->child_actions; a.root_value = q->root_value;
    PCB_GROUP_LAUNCH(k_gumbel_tree_leaves, a, (hipStream_t)q->stream);
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}
