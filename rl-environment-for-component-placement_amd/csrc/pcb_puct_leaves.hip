// pcb_puct_leaves.hip -- k_puct_leaves and its entry point pcbenv_puct_advance_leaves (include/pcbenv_leaves.h): the tree
// step of a leaf-parallel PUCT search, L descents per root and launch with pending (virtual) visits between them, and the
// backup of all L evaluations (what pcbenv/search.py:puct_search(leaves=L) does in tensor code).  Part of libpcbenv.so
// (CDNA4 / gfx950 only); a translation unit of its own, host side included, so that nothing here can change the build of
// k_puct_advance or of the other entry points.
//
// The step of one root is pcb_puct_leaves.h (leaves_init, leaves_select, leaves_absorb: the text
// tools/puct_leaves_check.cpp replays on the CPU); the kernel composes the same pieces with a group of G lanes per root
// (pcb_group.h: the mapping, the phases, the fence), child c of the current node in lane c as in k_puct_advance.  The L
// leaves of a root run one after the other inside its group.
//   select   lo, hi, c_puct and the root's own fields stay in registers across the leaves.  Per level ONE load round trip:
//            lane c loads, next to what the score of child c needs (visits, pending, value_sum, prior), that child's
//            terminal, num_children, first_child and action, so that the winner's are at hand -- a shuffle from its lane
//            -- when the descent enters it.  Lane 0 stores pending + 1 of a node as the descent leaves it, from the value
//            it has in a register; the winner's lane writes the path row.  A repeat (at most one per root and launch)
//            has added pending visits above the node it ended at: lane 0 takes them back along the parents.
//   absorb   per leaf as k_puct_advance: lanes c < k write one child slot each, lane 0 the node's fields and the backup
//            chain, one round trip per level, pending - 1 with it.  num_nodes, reward_lo and reward_hi stay in registers
//            across the leaves; the next leaf's `selected` is loaded while the current one is taken.
//   init     the slots of a root are contiguous: the lanes stride them.
// A leaf reads what the leaf before it stored through other lanes of the same wavefront -- pending in SELECT, the tree in
// ABSORB -- as a later phase reads an earlier one's: the same fence stands between leaves as between phases.
#include <hip/hip_runtime.h>

#include "pcb_group.h"
#include "pcb_tree_host.h"
#include "pcbenv_leaves.h"
#include "pcb_puct_leaves.h"

static_assert(PCBENV_TREE_INIT == pcb_puct::PHASE_INIT && PCBENV_TREE_ABSORB == pcb_puct::PHASE_ABSORB &&
              PCBENV_TREE_SELECT == pcb_puct::PHASE_SELECT && PCBENV_MAX_TREE_CHILDREN == pcb_puct::MAX_CHILDREN &&
              PCBENV_MAX_PUCT_LEAVES == pcb_puct_leaves::MAX_LEAVES, "pcbenv.h, pcbenv_leaves.h and pcb_puct_leaves.h name the same phases and bounds");
static_assert(sizeof(pcbenv_puct_leaves_request) == 240 && offsetof(pcbenv_puct_leaves_request, stream) == 232 &&
              offsetof(pcbenv_puct_leaves_request, num_leaves) == 40, "pcbenv/_leaves_lib.py:PcbenvPuctLeavesRequest");

namespace {

using namespace pcb_puct_leaves;
using pcb_group::BLOCK;

// what the kernel needs of a request
struct LeavesArgs {
    int phases, P, N, C, T, K, L;
    double c_puct;
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
    unsigned *errors;
};

template <int G> __device__ inline void init_phase(const Root &r, int *pending, int lane) {
    for (int s = lane; s < r.N; s += G) { init_slot(r, s); pending[s] = 0; }
    if (lane == 0) init_scalars(r);
}

// leaves_absorb, the new children of a leaf over the lanes; returns the error bits (the same in every lane)
template <int G> __device__ inline unsigned absorb_phase(const Root &r, const LeavesArgs &a, int *pending, int lane, int base) {
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
        if (l > 0) pcb_group::fence();
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

// leaves_select, child first_child + c of the current node in lane c
template <int G> __device__ inline unsigned select_phase(const Root &r, const LeavesArgs &a, int *pending, int lane, int base) {
    unsigned err = 0u;
    const double lo = *r.lo, hi = *r.hi, c_puct = a.c_puct;
    const int rows = a.P * a.L, row0 = r.p * a.L;
    // the root as every descent finds it: SELECT changes nothing of it but pending, which goes up by one per leaf
    const int term0 = r.terminal[0], k0 = r.num_children[0], fc0 = r.first_child[0], vis0 = r.visits[0];
    int pend0 = pending[0];
    int l = 0;
    for (; l < a.L; l++) {
        if (l > 0) pcb_group::fence();
        const int row = row0 + l;
        int node = 0, d = 0, term = term0, k = k0, fc = fc0, vis = vis0, pend = pend0;
        for (;; d++) {
            if (d >= r.T || stops(term, k)) break;
            if (!children_ok(fc, k, r.N, r.C)) { err |= ERR_TREE; break; }
            const bool mine = lane < k;
            const int ch = fc + (mine ? lane : 0);
            const int vis_c = r.visits[ch], pend_c = pending[ch], term_c = r.terminal[ch], k_c = r.num_children[ch], fc_c = r.first_child[ch];
            const int a0 = r.node_action[3 * ch], a1 = r.node_action[3 * ch + 1], a2 = r.node_action[3 * ch + 2];
            double s = mine ? leaves_score(r.value_sum[ch], vis_c, pend_c, r.prior[ch], lo, hi, c_puct, vis, pend) : neg_inf();
            PCB_GROUP_ARGMAX(G, mine, lane, s, c, beats)
            const int win = __shfl(c, base) & (G - 1);  // lane 0's verdict: one node per group whatever the scores were
            if (lane == 0) pending[node] = one_more(pend);
            if (lane == win) {
                a.paths[step_major(d, rows, row, 0)] = a0; a.paths[step_major(d, rows, row, 1)] = a1; a.paths[step_major(d, rows, row, 2)] = a2;
            }
            node = fc + win;
            term = __shfl(term_c, base + win); k = __shfl(k_c, base + win); fc = __shfl(fc_c, base + win);
            vis = __shfl(vis_c, base + win); pend = __shfl(pend_c, base + win);
        }
        if (repeats(term, k, pend)) {
            unsigned up = 0u;
            if (lane == 0) up = undo_pending(r, pending, node, d);
            err |= __shfl(up, base);
            break;
        }
        if (lane == 0) { pending[node] = one_more(pend); a.selected[row] = node; a.path_len[row] = d; }
        pend0 = one_more(pend0);
    }
    for (int j = l + lane; j < a.L; j += G) { a.selected[row0 + j] = -1; a.path_len[row0 + j] = -1; }  // behind a repeat
    return err;
}

template <int G> __global__ __launch_bounds__(BLOCK) void k_puct_leaves(const LeavesArgs a) {
    PCB_GROUP_ENTER(G, a);
    const Root r = root_of_group(a, (int)p, a.T);
    int *const pending = a.pending + (long long)p * a.N;
    PCB_GROUP_PHASES(a, init_phase<G>(r, pending, lane), absorb_phase<G>(r, a, pending, lane, base), select_phase<G>(r, a, pending, lane, base));
}

}  // namespace

// ---- pcbenv_puct_advance_leaves ----------------------------------------------------------------------------------
// As pcbenv_puct_advance: every argument check before a device is touched, the null handle last; then one launch.
extern "C" int pcbenv_puct_advance_leaves(const pcbenv *cenv, const pcbenv_puct_leaves_request *q) {
    using namespace pcb_tree_host;
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    PCB_TRY(check_search_request(env, q, "pcbenv_puct_leaves_request"));
    const Phases ph = phases_of(q->phases);
    if (q->num_leaves < 1 || q->num_leaves > PCBENV_MAX_PUCT_LEAVES) return fail(env, PCBENV_EINVAL, "num_leaves must be in [1, 64]");
    if ((long long)q->num_roots * q->num_leaves > 0x7fffffffLL) return fail(env, PCBENV_EINVAL, "num_roots * num_leaves must not exceed 2^31 - 1");
    PCB_TRY(check_puct_candidates(env, q, ph));
    if (q->reserved != 0 || q->reserved2 != 0) return fail(env, PCBENV_EINVAL, "reserved and reserved2 must be 0");
    PCB_TRY(check_puct_tree(env, q, !q->pending));
    PCB_TRY(check_exchange(env, q, ph));
    PCB_TRY(check_puct_inputs(env, q, ph));
    PCB_TRY(check_puct_doubles(env, q, ph.absorb ? q->value : 0));
    PCB_TRY(check_cand_prior(env, q, ph));
    PCB_TREE_CHECKS_END(env, q);
    LeavesArgs a;
    puct_search_args(a, q);
    a.L = q->num_leaves; a.pending = q->pending;
    PCB_GROUP_LAUNCH(k_puct_leaves, a, (hipStream_t)q->stream);
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}
