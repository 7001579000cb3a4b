// pcb_gumbel.hip -- k_gumbel_advance and its entry point pcbenv_gumbel_advance (include/pcbenv_gumbel.h): the tree step of
// a batch of searches whose root level is a Gumbel search with Sequential Halving, on the device (what
// pcbenv/search.py:gumbel_select_root and gumbel_choose do with a chain of gathers, masked argmaxes and three ln per child
// over [P, C]).  Part of libpcbenv.so (CDNA4 / gfx950 only); a translation unit of its own, host side included, so that
// nothing here can change the builds of the other kernels or of the other entry points.
//
// The rule of one root is pcb_gumbel.h (gumbel_begin, gumbel_select, gumbel_choose: the text tools/gumbel_check.cpp runs on
// the CPU) over pcb_puct.h; the kernel composes the same pieces on pcb_group.h's mapping: G = group_lanes(C) lanes per root,
// lane c at child c of the current node, 256 / G roots per workgroup.  Groups share nothing: no LDS, no barrier.
//   the root level   lane c computes g_c, logit_c and qhat_c of its child (three ln, some 90 double operations, no
//                    divergence: every lane of a group that is there runs them) and reads sim_visits[p, c].  The most
//                    visits among the children, and for CHOOSE the most simulations and the largest improved logit, are
//                    shuffle butterflies of a maximum -- an order-free operation; one ballot tells whether any child stands
//                    at the considered count; the argmax is pcb_group.h's.
//   choose           Z is formed by every lane of the group with the same loop over a lane shuffle of e, child after child:
//                    the order of the sum is the contract, so there is no tree reduction, and all lanes hold the same bits.
//   levels d >= 1    k_puct_advance's descent: pcb_puct_group.h's PCB_PUCT_DESCEND, from level 1 on.
//   absorb           k_puct_advance's absorb: pcb_puct_group.h's absorb_phase, over this unit's argument block.  Neither
//                    unit's instructions moved when the two copies became one (profiles/model_harness_refactor.txt).
#include <hip/hip_runtime.h>

#include "pcb_group.h"
#include "pcb_tree_host.h"
#include "pcbenv_gumbel.h"
#include "pcb_gumbel.h"
#include "pcb_puct_group.h"

static_assert(PCBENV_GUMBEL_BEGIN == pcb_gumbel::PHASE_BEGIN && PCBENV_GUMBEL_ABSORB == pcb_gumbel::PHASE_ABSORB &&
              PCBENV_GUMBEL_SELECT == pcb_gumbel::PHASE_SELECT && PCBENV_GUMBEL_CHOOSE == pcb_gumbel::PHASE_CHOOSE &&
              PCBENV_MAX_TREE_CHILDREN == pcb_gumbel::MAX_CHILDREN, "pcbenv_gumbel.h and pcb_gumbel.h name the same phases and bound");
static_assert(sizeof(pcbenv_gumbel_request) == 344 && offsetof(pcbenv_gumbel_request, stream) == 336 && offsetof(pcbenv_gumbel_request, c_puct) == 48 &&
              offsetof(pcbenv_gumbel_request, seed) == 72 && offsetof(pcbenv_gumbel_request, num_nodes) == 88 &&
              offsetof(pcbenv_gumbel_request, sim_index) == 256 && offsetof(pcbenv_gumbel_request, move_slot) == 280,
              "pcbenv/_gumbel_lib.py:PcbenvGumbelRequest");

namespace {

using namespace pcb_gumbel;
using namespace pcb_puct;
using pcb_group::BLOCK;
using pcb_group::fence;
using pcb_group::group_ballot;

// what the kernel needs of a request
struct GumbelArgs {
    int phases, P, N, C, T, K;
    double c_puct;
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

// what lane c holds of child fc + c of the root: its score, its improved logit and its counter
struct Child { double s, x; int sim; };
// k and fc have passed children_ok; a lane without a child holds numbers nobody reads
template <int G> __device__ inline Child root_child(const Root &r, const GumbelArgs &a, int lane, int k, int fc) {
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

template <int G> __device__ inline void begin_phase(const Root &r, const GumbelArgs &a, int lane) {
    if (lane == 0) a.sim_index[r.p] = 0;
    if (lane < r.C) a.sim_visits[(long long)r.p * r.C + lane] = 0;
}

// gumbel_select: the root level by the schedule, then puct_select's levels, child first_child + c of the current node in lane c
template <int G> __device__ inline unsigned select_phase(const Root &r, const GumbelArgs &a, int lane, int base) {
    unsigned err = 0u;
    const double lo = *r.lo, hi = *r.hi;
    int node = 0, d = 0;
    const int term0 = r.terminal[0], k0 = r.num_children[0], fc0 = r.first_child[0];
    bool go = !stops(term0, k0);
    if (go) {
        const int t = a.sim_index[r.p];
        if (!children_ok(fc0, k0, r.N, r.C) || t < 0) { err |= ERR_TREE; go = false; }
        else if (scheduled(t, a.q.n)) {
            const Child me = root_child<G>(r, a, lane, k0, fc0);
            const int v = a.considered[(long long)considered_candidates(a.q.Mc, k0) * a.q.n + t];
            const bool mine = lane < k0, at = mine && me.sim == v;
            const bool in = mine && (group_ballot<G>(at, base) == 0ull || at);
            double s = me.s;
            PCB_GROUP_ARGMAX(G, in, lane, s, c, beats)
            c = __shfl(c, base);  // lane 0's verdict
            node = fc0 + c;
            if (lane == c) a.sim_visits[(long long)r.p * r.C + lane] = one_more(me.sim);
            if (lane == 0) a.sim_index[r.p] = t + 1;
            if (lane < 3) a.paths[step_major(0, r.P, r.p, lane)] = r.node_action[3 * node + lane];
            d = 1;
        }
    }
    if (go) {
        PCB_PUCT_DESCEND(G, r, a, lane, base, lo, hi, node, d, err)
    }
    if (lane == 0) { a.selected[r.p] = node; a.path_len[r.p] = d; }
    return err;
}

// gumbel_choose, child first_child(0) + c in lane c
template <int G> __device__ inline unsigned choose_phase(const Root &r, const GumbelArgs &a, int lane, int base) {
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

template <int G> __global__ __launch_bounds__(BLOCK) void k_gumbel_advance(const GumbelArgs a) {
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

// ---- pcbenv_gumbel_advance ---------------------------------------------------------------------------------------
// As pcbenv_puct_advance: every argument check before a device is touched, the null handle last; then one launch.
extern "C" int pcbenv_gumbel_advance(const pcbenv *cenv, const pcbenv_gumbel_request *q) {
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
    GumbelArgs a;
    puct_search_args(a, q);
    a.q = Rule{q->c_puct, q->c_visit, q->c_scale, q->seed, q->step_index, q->first_root, q->num_simulations, q->max_considered};
    a.sim_index = q->sim_index; a.sim_visits = q->sim_visits; a.considered = q->considered;
    a.move_slot = q->move_slot; a.move_action = q->move_action; a.child_weights = q->child_weights; a.child_policy = q->child_policy;
    a.child_actions = q->child_actions; a.root_value = q->root_value;
    PCB_GROUP_LAUNCH(k_gumbel_advance, a, (hipStream_t)q->stream);
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}
