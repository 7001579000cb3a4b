// pcb_gumbel_leaves.hip -- k_gumbel_leaves and its entry point pcbenv_gumbel_advance_leaves (include/pcbenv_gumbel_leaves.h):
// the tree step of a batch of searches whose root level is a Gumbel search with Sequential Halving, L descents per root and
// launch with pending (virtual) visits between them, and the backup of all L evaluations (what
// pcbenv/search.py:gumbel_search(leaves=L) does in tensor code).  Part of libpcbenv.so (CDNA4 / gfx950 only); a translation
// unit of its own, host side included, so that nothing here can change the builds of k_gumbel_advance, k_puct_leaves or the
// other entry points: the pieces of pcb_gumbel.hip and pcb_puct_leaves.hip are composed here a second time, over this
// unit's argument block, and none of them moved.
//
// The rule of one root is pcb_gumbel_leaves.h (gumbel_leaves_select: the text tools/gumbel_leaves_check.cpp runs on the CPU)
// over pcb_gumbel.h and pcb_puct_leaves.h; the kernel composes the same pieces on pcb_group.h's mapping: G = group_lanes(C)
// lanes per root, lane c at child c of the current node, 256 / G roots per workgroup.  Groups share nothing: no LDS, no
// barrier.  Both parents are chains of dependent loads, not bandwidth or ALU work, so what a launch can know before its
// first leaf it loads before its first leaf:
//   root scores      lane c computes g_c, logit_c and sigma_c of its child once per launch (three ln and the butterfly of
//                    the most visits) and keeps the score for all L leaves: no leaf changes what the scores read.
//   root children    terminal, num_children, first_child, visits and the action of child c are loaded once into lane c;
//                    pending of a root child changes only through this group's own stores, so lane c counts it in a register.
//   counters         sim_visits[p, c] lives in lane c, sim_index in a uniform; each is stored once behind the last leaf.
//                    A repeat does not commit.
//   the table        the entries a launch can need are considered[m * n + t0 .. t0 + L - 1]: lane j of the group loads entry
//                    e * G + j for e < ceil(L / G), guarded by < n, in one round trip, and a leaf gets its entry by shuffle.
//   per leaf, root   one ballot (does any child stand at the considered count?), pcb_group.h's argmax, lane 0's verdict.
//   levels d >= 1    k_puct_leaves' level: one load round trip, the winner's fields by shuffle.
//   absorb           k_puct_leaves' absorb; begin and choose are k_gumbel_advance's.
// A leaf reads what the leaf before it stored through other lanes of the same wavefront: the same fence stands between
// leaves as between phases.
#include <hip/hip_runtime.h>

#include "pcb_group.h"
#include "pcb_tree_host.h"
#include "pcbenv_gumbel_leaves.h"
#include "pcb_gumbel_leaves.h"

static_assert(PCBENV_GUMBEL_BEGIN == pcb_gumbel::PHASE_BEGIN && PCBENV_GUMBEL_ABSORB == pcb_gumbel::PHASE_ABSORB &&
              PCBENV_GUMBEL_SELECT == pcb_gumbel::PHASE_SELECT && PCBENV_GUMBEL_CHOOSE == pcb_gumbel::PHASE_CHOOSE &&
              PCBENV_MAX_TREE_CHILDREN == pcb_gumbel::MAX_CHILDREN && PCBENV_MAX_PUCT_LEAVES == pcb_puct_leaves::MAX_LEAVES,
              "pcbenv_gumbel.h, pcbenv_leaves.h, pcb_gumbel.h and pcb_puct_leaves.h name the same phases and bounds");
static_assert(sizeof(pcbenv_gumbel_leaves_request) == 360 && offsetof(pcbenv_gumbel_leaves_request, stream) == 352 &&
              offsetof(pcbenv_gumbel_leaves_request, c_puct) == 48 && offsetof(pcbenv_gumbel_leaves_request, seed) == 72 &&
              offsetof(pcbenv_gumbel_leaves_request, num_leaves) == 88 && offsetof(pcbenv_gumbel_leaves_request, num_nodes) == 96 &&
              offsetof(pcbenv_gumbel_leaves_request, pending) == 200 && offsetof(pcbenv_gumbel_leaves_request, sim_index) == 272 &&
              offsetof(pcbenv_gumbel_leaves_request, move_slot) == 296, "pcbenv/_gumbel_leaves_lib.py:PcbenvGumbelLeavesRequest");

namespace {

using namespace pcb_gumbel_leaves;
using pcb_gumbel::completed_q;
using pcb_gumbel::draw_base;
using pcb_gumbel::gumbel;
using pcb_gumbel::ieee_exp;
using pcb_gumbel::improved;
using pcb_gumbel::larger;
using pcb_gumbel::logit;
using pcb_gumbel::root_mean;
using pcb_gumbel::score;
using pcb_gumbel::sigma;
using pcb_gumbel::weight;
using pcb_group::BLOCK;
using pcb_group::fence;
using pcb_group::group_ballot;

// what the kernel needs of a request
struct GumbelLeavesArgs {
    int phases, P, N, C, T, K, L;
    double c_puct;
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

// what lane c holds of child fc + c of the root: its score, its improved logit and its counter
struct Child { double s, x; int sim; };
// k and fc have passed children_ok; a lane without a child holds numbers nobody reads
template <int G> __device__ inline Child root_child(const Root &r, const GumbelLeavesArgs &a, int lane, int k, int fc) {
    const bool mine = lane < k;
    const int ch = fc + (mine ? lane : 0);
    const double lo = *r.lo, hi = *r.hi, vbar = root_mean(r.value_sum[0], r.visits[0], lo);
    const int n_c = r.visits[ch];
    const int sim = mine ? a.sim_visits[(long long)r.p * r.C + lane] : 0;
    const double pr = r.prior[ch], sum = r.value_sum[ch];
    const int most = group_max<G>(mine ? n_c : INT_MIN);
    const double lg = logit(pr), sg = sigma(completed_q(sum, n_c, vbar, lo, hi), most, a.q.c_visit, a.q.c_scale);
    const double g = gumbel(draw_base(a.q.seed, a.q.first_root + r.p, a.q.step_index), lane);
    return Child{score(g, lg, sg), improved(lg, sg), sim};
}

template <int G> __device__ inline void begin_phase(const Root &r, const GumbelLeavesArgs &a, int lane) {
    if (lane == 0) a.sim_index[r.p] = 0;
    if (lane < r.C) a.sim_visits[(long long)r.p * r.C + lane] = 0;
}

// leaves_absorb, the new children of a leaf over the lanes; returns the error bits (the same in every lane)
template <int G> __device__ inline unsigned absorb_phase(const Root &r, const GumbelLeavesArgs &a, int *pending, int lane, int base) {
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

// gumbel_leaves_select, child first_child + c of the current node in lane c
template <int G> __device__ inline unsigned select_phase(const Root &r, const GumbelLeavesArgs &a, int *pending, int lane, int base) {
    constexpr int E = MAX_LEAVES / G;  // table entries a lane can be asked for: ceil(L / G) of them are loaded
    unsigned err = 0u;
    const double lo = *r.lo, hi = *r.hi, c_puct = a.c_puct;
    const int rows = a.P * a.L, row0 = r.p * a.L, n = a.q.n;
    // the root as every descent finds it: SELECT changes nothing of it but pending, which goes up by one per leaf
    const int term0 = r.terminal[0], k0 = r.num_children[0], fc0 = r.first_child[0], vis0 = r.visits[0];
    int pend0 = pending[0];
    const int t0 = a.sim_index[r.p];
    const bool halts = stops(term0, k0);
    int l = 0;
    if (halts || !children_ok(fc0, k0, r.N, r.C) || t0 < 0) {  // no descent: the root itself, once
        if (!halts) err |= ERR_TREE;
        if (lane == 0) { pending[0] = one_more(pend0); a.selected[row0] = 0; a.path_len[row0] = 0; }
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
        const int ch0 = fc0 + (mine0 ? lane : 0);
        const int vis_r = r.visits[ch0], term_r = r.terminal[ch0], k_r = r.num_children[ch0], fc_r = r.first_child[ch0];
        const int a0_r = r.node_action[3 * ch0], a1_r = r.node_action[3 * ch0 + 1], a2_r = r.node_action[3 * ch0 + 2];
        int pend_r = pending[ch0];
        const Child me = root_child<G>(r, a, lane, k0, fc0);
        int sim = me.sim, t = t0;
        for (; l < a.L; l++) {
            if (l > 0) fence();
            const int row = row0 + l;
            const bool on_schedule = t < n;
            if (!on_schedule && l > 0) break;  // out of budget: no evaluator row for an unscheduled descent
            int node = 0, d = 0, term = term0, k = k0, fc = fc0, vis = vis0, pend = pend0, win0 = 0;
            if (on_schedule) {
                const int i = t - t0;  // the leaves before this one committed i simulations
                int mine_v = 0;
                #pragma unroll
                for (int e = 0; e < E; e++) mine_v = (i / G == e) ? table[e] : mine_v;
                const int v = __shfl(mine_v, base + (i & (G - 1)));
                const bool at = mine0 && sim == v;
                const bool in = mine0 && (group_ballot<G>(at, base) == 0ull || at);
                double s = me.s;
                PCB_GROUP_ARGMAX(G, in, lane, s, c, beats)
                win0 = __shfl(c, base) & (G - 1);  // lane 0's verdict: one node per group whatever the scores were
                if (lane == 0) pending[0] = one_more(pend0);
                if (lane == win0) {
                    a.paths[step_major(0, rows, row, 0)] = a0_r; a.paths[step_major(0, rows, row, 1)] = a1_r; a.paths[step_major(0, rows, row, 2)] = a2_r;
                }
                node = fc0 + win0;
                term = __shfl(term_r, base + win0); k = __shfl(k_r, base + win0); fc = __shfl(fc_r, base + win0);
                vis = __shfl(vis_r, base + win0); pend = __shfl(pend_r, base + win0);
                d = 1;
            }
            for (;; d++) {
                if (d >= r.T || stops(term, k)) break;
                if (!children_ok(fc, k, r.N, r.C)) { err |= ERR_TREE; break; }
                const bool mine = lane < k;
                const int ch = fc + (mine ? lane : 0);
                const int vis_c = r.visits[ch], pend_c = pending[ch], term_c = r.terminal[ch], k_c = r.num_children[ch], fc_c = r.first_child[ch];
                const int a0 = r.node_action[3 * ch], a1 = r.node_action[3 * ch + 1], a2 = r.node_action[3 * ch + 2];
                double s = mine ? leaves_score(r.value_sum[ch], vis_c, pend_c, r.prior[ch], lo, hi, c_puct, vis, pend) : neg_inf();
                PCB_GROUP_ARGMAX(G, mine, lane, s, c, beats)
                const int win = __shfl(c, base) & (G - 1);  // lane 0's verdict
                if (lane == 0) pending[node] = one_more(pend);
                if (lane == win) {
                    a.paths[step_major(d, rows, row, 0)] = a0; a.paths[step_major(d, rows, row, 1)] = a1; a.paths[step_major(d, rows, row, 2)] = a2;
                }
                node = fc + win;
                term = __shfl(term_c, base + win); k = __shfl(k_c, base + win); fc = __shfl(fc_c, base + win);
                vis = __shfl(vis_c, base + win); pend = __shfl(pend_c, base + win);
            }
            if (repeats(term, k, pend)) {  // it consumes no simulation: the counters stay as they were before this leaf
                unsigned up = 0u;
                if (lane == 0) up = undo_pending(r, pending, node, d);
                err |= __shfl(up, base);
                break;
            }
            if (lane == 0) { pending[node] = one_more(pend); a.selected[row] = node; a.path_len[row] = d; }
            pend0 = one_more(pend0);
            if (on_schedule) {
                if (lane == win0) { sim = pcb_gumbel::one_more(sim); pend_r = one_more(pend_r); }  // the root child was left or reached: one pending visit
                t += 1;
            }
        }
        if (t != t0) {
            if (mine0 && sim != me.sim) a.sim_visits[(long long)r.p * r.C + lane] = sim;
            if (lane == 0) a.sim_index[r.p] = t;
        }
    }
    for (int j = l + lane; j < a.L; j += G) { a.selected[row0 + j] = -1; a.path_len[row0 + j] = -1; }  // no leaf
    return err;
}

// gumbel_choose, child first_child(0) + c in lane c
template <int G> __device__ inline unsigned choose_phase(const Root &r, const GumbelLeavesArgs &a, int lane, int base) {
    unsigned err = 0u;
    int k = r.num_children[0];
    const int fc = r.first_child[0], visits0 = r.visits[0];
    const double sum0 = r.value_sum[0];
    if (k != 0 && !children_ok(fc, k, r.N, r.C)) { err |= ERR_TREE; k = 0; }
    const bool mine = lane < k;
    int act[3] = {0, 0, 0};
    double pi = 0.0;
    int c = 0;
    if (k > 0) {  // the whole group
        const Child me = root_child<G>(r, a, lane, k, fc);
        const int ch = fc + (mine ? lane : 0);
        #pragma unroll
        for (int i = 0; i < 3; i++) act[i] = mine ? r.node_action[3 * ch + i] : 0;
        const int most = group_max<G>(mine ? me.sim : INT_MIN);
        const double mx = group_max<G>(mine ? me.x : neg_inf());
        const double e = mine ? ieee_exp(me.x - mx) : 0.0;
        double Z = 0.0;
        #pragma unroll
        for (int b = 0; b < G; b++) {
            const double eb = __shfl(e, b, G);
            Z = b < k ? Z + eb : Z;
        }
        pi = e / Z;
        const bool in = mine && me.sim == most;
        double s = me.s;
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

template <int G> __global__ __launch_bounds__(BLOCK) void k_gumbel_leaves(const GumbelLeavesArgs a) {
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

// ---- pcbenv_gumbel_advance_leaves --------------------------------------------------------------------------------
// As pcbenv_gumbel_advance: every argument check before a device is touched, the null handle last; then one launch.
extern "C" int pcbenv_gumbel_advance_leaves(const pcbenv *cenv, const pcbenv_gumbel_leaves_request *q) {
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
    GumbelLeavesArgs a;
    puct_search_args(a, q);
    a.L = q->num_leaves; a.pending = q->pending;
    a.q = Rule{q->c_puct, q->c_visit, q->c_scale, q->seed, q->step_index, q->first_root, q->num_simulations, q->max_considered};
    a.sim_index = q->sim_index; a.sim_visits = q->sim_visits; a.considered = q->considered;
    a.move_slot = q->move_slot; a.move_action = q->move_action; a.child_weights = q->child_weights; a.child_policy = q->child_policy;
    a.child_actions = q->child_actions; a.root_value = q->root_value;
    PCB_GROUP_LAUNCH(k_gumbel_leaves, a, (hipStream_t)q->stream);
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}
