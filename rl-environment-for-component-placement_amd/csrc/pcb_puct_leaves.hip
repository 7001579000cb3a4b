// pcb_puct_leaves.hip -- k_puct_leaves and its entry point pcbenv_puct_advance_leaves (include/pcbenv_leaves.h): the tree
// step of a leaf-parallel PUCT search, L descents per root and launch with pending (virtual) visits between them, and the
// backup of all L evaluations (what pcbenv/search.py:puct_search(leaves=L) does in tensor code).  Part of libpcbenv.so
// (CDNA4 / gfx950 only); a translation unit of its own, host side included, so that nothing here can change the build of
// k_puct_advance or of the other entry points.
//
// The step of one root is pcb_puct_leaves.h (leaves_init, leaves_select, leaves_absorb: the text
// tools/puct_leaves_check.cpp replays on the CPU); the kernel composes the same pieces with k_puct_advance's mapping: a
// group of G lanes per root, G the power of two >= max(C, 4), child c of the current node in lane c, the argmax a shuffle
// butterfly.  Groups share nothing: no LDS, no barrier, and a group whose root does not exist exits whole.  The L leaves
// of a root run one after the other inside its group.
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
// ABSORB -- as a later phase reads an earlier one's: a wavefront-scope fence between leaves and between phases keeps the
// compiler from moving those loads up; the memory operations of one wavefront reach the cache in order.
#include <hip/hip_runtime.h>

#include "pcb_host.h"
#include "pcbenv_leaves.h"
#include "pcb_puct_leaves.h"

static_assert(PCBENV_TREE_INIT == pcb_puct::PHASE_INIT && PCBENV_TREE_ABSORB == pcb_puct::PHASE_ABSORB &&
              PCBENV_TREE_SELECT == pcb_puct::PHASE_SELECT && PCBENV_MAX_TREE_CHILDREN == pcb_puct::MAX_CHILDREN &&
              PCBENV_MAX_PUCT_LEAVES == pcb_puct_leaves::MAX_LEAVES, "pcbenv.h, pcbenv_leaves.h and pcb_puct_leaves.h name the same phases and bounds");
static_assert(sizeof(pcbenv_puct_leaves_request) == 240 && offsetof(pcbenv_puct_leaves_request, stream) == 232 &&
              offsetof(pcbenv_puct_leaves_request, num_leaves) == 40, "pcbenv/_leaves_lib.py:PcbenvPuctLeavesRequest");

namespace {

using namespace pcb_puct_leaves;
constexpr int BLOCK = 256;

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

__device__ inline Root root_of_group(const LeavesArgs &a, int p) {
    const long long s = (long long)p * a.N;
    return Root{a.N, a.C, a.T, a.P, p, a.num_nodes + p, a.parent + s, a.depth + s, a.visits + s, a.num_children + s, a.first_child + s,
                a.node_action + 3 * s, a.prior + s, a.value_sum + s, a.value_max + s, a.terminal + s, a.lo + p, a.hi + p};
}

__device__ inline void leaf_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

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
        if (l > 0) leaf_fence();
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
        if (l > 0) leaf_fence();
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
            int c = mine ? lane : MAX_CHILDREN + lane;  // a lane without a child loses against any child, whatever its score
            #pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) {
                const double so = __shfl_xor(s, o);
                const int co = __shfl_xor(c, o);
                const bool other = co < MAX_CHILDREN && (c >= MAX_CHILDREN || beats(so, co, s, c));
                s = other ? so : s;
                c = other ? co : c;
            }
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
    static_assert(G >= 4 && G <= 64 && (G & (G - 1)) == 0, "a group is a power-of-two part of a wavefront");
    const unsigned p = blockIdx.x * (BLOCK / G) + threadIdx.x / G;
    if (p >= (unsigned)a.P) return;
    const int lane = threadIdx.x % G, base = (threadIdx.x & 63) - lane;
    const Root r = root_of_group(a, (int)p);
    int *const pending = a.pending + (long long)p * a.N;
    unsigned err = 0u;
    if (a.phases & PHASE_INIT) {
        init_phase<G>(r, pending, lane);
        leaf_fence();
    }
    if (a.phases & PHASE_ABSORB) {
        err |= absorb_phase<G>(r, a, pending, lane, base);
        leaf_fence();
    }
    if (a.phases & PHASE_SELECT) err |= select_phase<G>(r, a, pending, lane, base);
    if (err != 0u && lane == 0 && a.errors) atomicOr(a.errors, err);
}

int group_lanes(int C) { int g = 4; while (g < C) g <<= 1; return g; }

}  // namespace

// ---- pcbenv_puct_advance_leaves ----------------------------------------------------------------------------------
// As pcbenv_puct_advance: every argument check before a device is touched, the null handle last; then one launch.
extern "C" int pcbenv_puct_advance_leaves(const pcbenv *cenv, const pcbenv_puct_leaves_request *q) {
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    if (!q) return fail(env, PCBENV_EINVAL, "null request");
    if (q->struct_size != (uint32_t)sizeof(pcbenv_puct_leaves_request)) return fail(env, PCBENV_EINVAL, "struct_size is not sizeof(pcbenv_puct_leaves_request)");
    const int ph = q->phases;
    const bool init = ph & PCBENV_TREE_INIT, absorb = ph & PCBENV_TREE_ABSORB, select = ph & PCBENV_TREE_SELECT;
    if (ph == 0 || (ph & ~(PCBENV_TREE_INIT | PCBENV_TREE_ABSORB | PCBENV_TREE_SELECT)) != 0) return fail(env, PCBENV_EINVAL, "phases must be a non-empty set of INIT, ABSORB, SELECT");
    if (init && absorb) return fail(env, PCBENV_EINVAL, "phases: INIT cannot be combined with ABSORB");
    if (q->num_roots < 0) return fail(env, PCBENV_EINVAL, "num_roots must not be negative");
    if (q->capacity < 1) return fail(env, PCBENV_EINVAL, "capacity must be at least 1");
    if (q->max_children < 1 || q->max_children > PCBENV_MAX_TREE_CHILDREN) return fail(env, PCBENV_EINVAL, "max_children must be in [1, 64]");
    if (q->max_steps < 1) return fail(env, PCBENV_EINVAL, "max_steps must be at least 1");
    if (q->num_leaves < 1 || q->num_leaves > PCBENV_MAX_PUCT_LEAVES) return fail(env, PCBENV_EINVAL, "num_leaves must be in [1, 64]");
    if ((long long)q->num_roots * q->num_leaves > 0x7fffffffLL) return fail(env, PCBENV_EINVAL, "num_roots * num_leaves must not exceed 2^31 - 1");
    if (absorb && q->num_candidates < 1) return fail(env, PCBENV_EINVAL, "num_candidates must be at least 1 with ABSORB");
    if (q->reserved != 0 || q->reserved2 != 0) return fail(env, PCBENV_EINVAL, "reserved and reserved2 must be 0");
    if (!q->num_nodes || !q->parent || !q->depth || !q->visits || !q->num_children || !q->first_child || !q->node_action || !q->prior ||
        !q->value_sum || !q->value_max || !q->terminal || !q->reward_lo || !q->reward_hi || !q->pending) return fail(env, PCBENV_EINVAL, "null tree tensor");
    if ((absorb || select) && !q->selected) return fail(env, PCBENV_EINVAL, "null selected");
    if (select && (!q->path_len || !q->paths)) return fail(env, PCBENV_EINVAL, "null path_len or paths with SELECT");
    if (absorb && (!q->value || !q->leaf_terminal || !q->cand_count || !q->cand_actions || !q->cand_prior))
        return fail(env, PCBENV_EINVAL, "null value, leaf_terminal, cand_count, cand_actions or cand_prior with ABSORB");
    const uintptr_t doubles = (uintptr_t)q->prior | (uintptr_t)q->value_sum | (uintptr_t)q->value_max | (uintptr_t)q->reward_lo |
                              (uintptr_t)q->reward_hi | (absorb ? (uintptr_t)q->value : 0);
    if ((doubles & 7u) != 0) return fail(env, PCBENV_EINVAL, "the float64 tensors must be 8-byte aligned");
    if (absorb && ((uintptr_t)q->cand_prior & 3u) != 0) return fail(env, PCBENV_EINVAL, "cand_prior must be 4-byte aligned");
    if (!env) return fail(0, PCBENV_EINVAL, "null handle");
    if (q->num_roots == 0) return PCBENV_OK;
    DEVICE_GUARD(env);
    LeavesArgs a;
    a.phases = ph; a.P = q->num_roots; a.N = q->capacity; a.C = q->max_children; a.T = q->max_steps; a.K = q->num_candidates; a.L = q->num_leaves;
    a.c_puct = q->c_puct;
    a.num_nodes = q->num_nodes; a.parent = q->parent; a.depth = q->depth; a.visits = q->visits; a.num_children = q->num_children;
    a.first_child = q->first_child; a.node_action = q->node_action; a.prior = q->prior; a.value_sum = q->value_sum; a.value_max = q->value_max;
    a.terminal = q->terminal; a.lo = q->reward_lo; a.hi = q->reward_hi; a.pending = q->pending; a.selected = q->selected; a.path_len = q->path_len;
    a.paths = q->paths; a.value = q->value; a.leaf_terminal = q->leaf_terminal; a.cand_count = q->cand_count; a.cand_actions = q->cand_actions;
    a.cand_prior = q->cand_prior; a.errors = (unsigned *)q->errors_dev;
    const int G = group_lanes(a.C);
    const unsigned grid = (unsigned)(((long long)a.P + BLOCK / G - 1) / (BLOCK / G));
    hipStream_t s = (hipStream_t)q->stream;
    switch (G) {
    case 4: hipLaunchKernelGGL(k_puct_leaves<4>, dim3(grid), dim3(BLOCK), 0, s, a); break;
    case 8: hipLaunchKernelGGL(k_puct_leaves<8>, dim3(grid), dim3(BLOCK), 0, s, a); break;
    case 16: hipLaunchKernelGGL(k_puct_leaves<16>, dim3(grid), dim3(BLOCK), 0, s, a); break;
    case 32: hipLaunchKernelGGL(k_puct_leaves<32>, dim3(grid), dim3(BLOCK), 0, s, a); break;
    default: hipLaunchKernelGGL(k_puct_leaves<64>, dim3(grid), dim3(BLOCK), 0, s, a); break;
    }
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}
