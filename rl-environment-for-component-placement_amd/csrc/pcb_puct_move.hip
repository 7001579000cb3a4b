// pcb_puct_move.hip -- k_puct_move and its entry point pcbenv_puct_move (include/pcbenv_move.h): the move of a batch of
// PUCT trees and the compaction of the subtree below it, on the device (what pcbenv/search.py:puct_choose and puct_reroot
// do with a pointer-jumping loop, a cumsum and a dozen scatters over [P, N]).  Part of libpcbenv.so (CDNA4 / gfx950
// only); a translation unit of its own, host side included, so that nothing here can change the builds of the other
// kernels or of the other entry points.
//
// The step of one root is pcb_puct_move.h (move_choose, move_reroot: the text tools/puct_move_check.cpp runs on the CPU);
// the kernel composes the same pieces with one wavefront per root, four roots per 256-thread workgroup.  Wavefronts share
// nothing: no LDS, no barrier, and a wavefront whose root does not exist exits whole.
//   choose   lane c owns child first_child(0) + c: consecutive slots, one load per field.  The most-visited child is a
//            shuffle butterfly, the proportional pick a 64-bit prefix sum over the lanes and one ballot.
//   reroot   a stream over the n used slots in chunks of 64, lane l at slot chunk + l, so every tensor's loads and
//            stores are contiguous; a lane holds four chunks (a span) at a time, so that a round trip to memory is paid once
//            per 256 slots: the work is a chain of dependent round trips per wavefront, and with one wavefront per root
//            there are only four wavefronts per SIMD at 4 096 roots to hide them.  Three passes, and the tree is written
//            by the last one only (all or nothing):
//            1. ranks: a slot is kept if it is m or its parent is kept.  A parent below the span has its verdict in remap
//               already (one gather); one in an earlier chunk of the span has it in that chunk's ballot, a register; one
//               inside the chunk is another lane.  That last case is resolved by an in-chunk fix-point over __shfl with
//               pointer doubling: at most 6 rounds of two ds_bpermute_b32 each, all in registers (the generated loop is two
//               ds_bpermute, three compares and a ballot) -- against walking ancestors down to depth(m), which is up to T
//               DEPENDENT global loads per slot: a C = 1 chain pays all of them in every lane.  The kept flags are single
//               bits, so the rank is the ballot's population count below the lane (v_mbcnt) plus a running base, not a DPP
//               scan of integers; remap gets the rank.
//            2. the child ranges of the kept nodes, checked against n, C and remap.
//            3. the move: a span's nodes are loaded whole, then stored at their ranks; the slots given up get INIT values.
//               In place is safe for a single wavefront going up: a span's stores land at or below its own slots, never
//               in a later span.
// A later pass reads what an earlier one stored through other lanes of the same wavefront, and a span's loads must all
// be done before its stores: a wavefront-scope fence between them keeps the compiler from moving loads across.
#include <hip/hip_runtime.h>

#include "pcb_group.h"
#include "pcb_tree_host.h"
#include "pcbenv_move.h"
#include "pcb_puct_move.h"

static_assert(PCBENV_MOVE_CHOOSE == pcb_move::PHASE_CHOOSE && PCBENV_MOVE_REROOT == pcb_move::PHASE_REROOT &&
              PCBENV_MOVE_GREEDY == pcb_move::MODE_GREEDY && PCBENV_MOVE_PROPORTIONAL == pcb_move::MODE_PROPORTIONAL &&
              PCBENV_MAX_TREE_CHILDREN == pcb_move::MAX_CHILDREN, "pcbenv_move.h and pcb_puct_move.h name the same phases and modes");
static_assert(sizeof(pcbenv_puct_move_request) == 224 && offsetof(pcbenv_puct_move_request, stream) == 216 &&
              offsetof(pcbenv_puct_move_request, seed) == 32, "pcbenv/_move_lib.py:PcbenvPuctMoveRequest");

namespace {

using namespace pcb_move;
using pcb_group::BLOCK;
using pcb_group::fence;
constexpr int LANES = 64, UNROLL = 4, SPAN = UNROLL * LANES;  // a lane holds UNROLL slots of a span at a time
static_assert(MAX_CHILDREN <= LANES, "one lane per child of the root");

// what the kernel needs of a request
struct MoveArgs {
    int phases, P, N, C, mode, first_root;
    uint64_t seed, step_index;
    int *num_nodes, *parent, *depth, *visits, *num_children, *first_child, *node_action;
    double *prior, *value_sum, *value_max;
    uint8_t *terminal;
    double *lo, *hi;
    int *move_slot, *move_action, *child_visits, *child_actions;
    double *root_value;
    int *remap;
    const uint8_t *reset;
    unsigned *errors;
};

// move_choose, child first_child(0) + c in lane c; returns move_slot (the same in every lane)
__device__ inline int choose_phase(const Root &r, const MoveArgs &a, int lane, unsigned *err) {
    int k = r.num_children[0];
    const int fc = r.first_child[0], visits0 = r.visits[0];
    const double sum0 = r.value_sum[0];
    if (k != 0 && !children_ok(fc, k, r.N, r.C)) { *err |= ERR_TREE; k = 0; }
    const bool mine = lane < k;
    const int ch = mine ? fc + lane : 0;
    const int v = mine ? r.visits[ch] : 0;
    int act[3];
    #pragma unroll
    for (int i = 0; i < 3; i++) act[i] = mine ? r.node_action[3 * ch + i] : 0;
    if (lane < r.C) {
        const long long row = (long long)r.p * r.C + lane;
        a.child_visits[row] = v;
        #pragma unroll
        for (int i = 0; i < 3; i++) a.child_actions[3 * row + i] = act[i];
    }
    int bv = v;
    PCB_GROUP_ARGMAX(LANES, mine, lane, bv, bc, more_visits)
    bc = __shfl(bc, 0);
    long long prefix = v;
    #pragma unroll
    for (int o = 1; o < LANES; o <<= 1) {
        const long long t = __shfl_up(prefix, o);
        if (lane >= o) prefix += t;
    }
    const long long total = __shfl(prefix, LANES - 1);
    if (k > 0 && draws(a.mode, total)) {
        const long long at = draw_rank(draw_hi32(a.seed, a.first_root + r.p, a.step_index), total);
        const unsigned long long hit = __ballot(mine && prefix > at);
        if (hit != 0ull) bc = __ffsll((long long)hit) - 1;
    }
    const int src = k > 0 ? bc : 0;
    #pragma unroll
    for (int i = 0; i < 3; i++) act[i] = k > 0 ? __shfl(act[i], src) : 0;
    const int slot = k > 0 ? fc + bc : -1;
    if (lane == 0) {
        a.move_slot[r.p] = slot;
        a.root_value[r.p] = mean_value(sum0, visits0);
    }
    if (lane < 3) a.move_action[3 * (long long)r.p + lane] = lane == 0 ? act[0] : lane == 1 ? act[1] : act[2];
    return slot;
}

__device__ inline void fill_remap_lanes(int *remap, int N, int lane, int v) { for (int s = lane; s < N; s += LANES) remap[s] = v; }

// move_reroot, slot chunk + l in lane l; returns the error bits (the same in every lane)
__device__ inline unsigned reroot_phase(const Root &r, const MoveArgs &a, int lane, int m) {
    int *remap = a.remap + (long long)r.p * r.N;
    const int reset = a.reset ? a.reset[r.p] : 0;
    if (resets(reset, m)) {
        for (int s = lane; s < r.N; s += LANES) { init_slot(r, s); remap[s] = -1; }
        if (lane == 0) init_scalars(r);
        return 0u;
    }
    const int n = *r.num_nodes;
    if (!count_ok(n, r.N) || !move_ok(m, n)) { fill_remap_lanes(remap, r.N, lane, -1); return ERR_TREE; }
    if (m == 0) {
        for (int s = lane; s < r.N; s += LANES) remap[s] = s < n ? s : -1;
        return 0u;
    }
    // 1. the ranks of the kept slots, a span of UNROLL chunks per round
    bool ok = true;
    int count = 0;
    for (int first = 0; first < r.N; first += SPAN) {
        int up[UNROLL], verdict[UNROLL], ask[UNROLL];
        bool bad = false;
        #pragma unroll
        for (int u = 0; u < UNROLL; u++) {  // one round trip: the parents of the span
            const int s = first + u * LANES + lane;
            up[u] = s >= 1 && s < n ? r.parent[s] : -1;
        }
        #pragma unroll
        for (int u = 0; u < UNROLL; u++) {  // a second one: the verdicts of the parents below the span, which remap holds
            const int s = first + u * LANES + lane;
            verdict[u] = OUT;
            ask[u] = lane;  // the lane of the slot's own chunk that holds its parent
            if (s >= 1 && s < n) {
                if (!parent_ok(up[u], s)) bad = true;
                else {
                    verdict[u] = kept_at_sight(s, m, up[u]);
                    if (verdict[u] == ASK_PARENT && up[u] < first) verdict[u] = remap[up[u]] >= 0 ? IN : OUT;
                }
            }
        }
        if (__any(bad)) { ok = false; break; }
        unsigned long long in[UNROLL];  // the kept slots of the span's chunks so far, a bit per lane
        #pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const int chunk = first + u * LANES, s = chunk + lane;
            if (verdict[u] == ASK_PARENT) {
                if (up[u] < chunk) {  // the parent is in an earlier chunk of this span
                    unsigned long long theirs = 0ull;
                    #pragma unroll
                    for (int w = 0; w < u; w++) theirs = (up[u] - first) / LANES == w ? in[w] : theirs;
                    verdict[u] = (theirs >> ((up[u] - first) % LANES)) & 1ull ? IN : OUT;
                } else ask[u] = up[u] - chunk;
            }
            // the parent is another lane: the lowest lane still asking has a parent that knows, and every round halves the way to one
            while (__any(verdict[u] == ASK_PARENT)) {
                const int theirs = __shfl(verdict[u], ask[u]), next = __shfl(ask[u], ask[u]);
                if (verdict[u] == ASK_PARENT) {
                    if (theirs != ASK_PARENT) verdict[u] = theirs;
                    else ask[u] = next;
                }
            }
            in[u] = __ballot(verdict[u] == IN);
            if (s < r.N) remap[s] = verdict[u] == IN ? count + __popcll(in[u] & ((1ull << lane) - 1ull)) : -1;
            count += __popcll(in[u]);
        }
        fence();
    }
    // 2. the child ranges of the kept nodes
    const int first_chunk = m & ~(LANES - 1);
    for (int first = first_chunk; ok && first < n; first += SPAN) {
        int k[UNROLL], fc[UNROLL];
        bool kept[UNROLL], bad = false;
        #pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const int s = first + u * LANES + lane;
            kept[u] = false; k[u] = 0; fc[u] = -1;
            if (s < n) { kept[u] = remap[s] >= 0; k[u] = r.num_children[s]; fc[u] = r.first_child[s]; }
        }
        #pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            if (!kept[u]) continue;
            if (!kept_children_ok(fc[u], k[u], n, r.C)) bad = true;
            else if (k[u] > 0 && !range_kept(remap[fc[u]], remap[fc[u] + k[u] - 1], k[u])) bad = true;
        }
        if (__any(bad)) ok = false;
    }
    if (!ok) { fill_remap_lanes(remap, r.N, lane, -1); return ERR_TREE; }
    // 3. the move, going up; the slots given up start below m's chunk when few are kept
    const int depth_m = r.depth[m];
    fence();
    for (int first = (count < m ? count : m) & ~(LANES - 1); first < n; first += SPAN) {
        int to[UNROLL], parent_rank[UNROLL], child_rank[UNROLL];
        Node x[UNROLL];
        #pragma unroll
        for (int u = 0; u < UNROLL; u++) {  // one round trip: every node of the span, kept or not
            const int s = first + u * LANES + lane;
            to[u] = -1;
            x[u] = Node{};
            if (s >= m && s < n) { to[u] = remap[s]; x[u] = load_node(r, s); }
        }
        #pragma unroll
        for (int u = 0; u < UNROLL; u++) {  // a second one: the new names of the kept nodes' links, which pass 1 and 2 have checked
            const int s = first + u * LANES + lane;
            parent_rank[u] = to[u] >= 0 && s != m ? remap[x[u].parent] : -1;
            child_rank[u] = to[u] >= 0 && x[u].num_children > 0 ? remap[x[u].first_child] : -1;
        }
        fence();
        #pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const int s = first + u * LANES + lane;
            if (to[u] >= 0) store_node(r, to[u], rerooted(x[u], s == m, parent_rank[u], child_rank[u], depth_m));
            if (s >= count && s < n) init_slot(r, s);
        }
        fence();
    }
    if (lane == 0) *r.num_nodes = count;
    return 0u;
}

__global__ __launch_bounds__(BLOCK) void k_puct_move(const MoveArgs a) {
    const unsigned p = blockIdx.x * (BLOCK / LANES) + threadIdx.x / LANES;
    if (p >= (unsigned)a.P) return;
    const int lane = threadIdx.x % LANES;
    const Root r = pcb_puct::root_of_group(a, (int)p, 0);
    unsigned err = 0u;
    int m = 0;
    if (a.phases & PHASE_CHOOSE) {
        m = choose_phase(r, a, lane, &err);
        fence();
    } else m = a.move_slot[p];
    if (a.phases & PHASE_REROOT) err |= reroot_phase(r, a, lane, m);
    if (err != 0u && lane == 0 && a.errors) atomicOr(a.errors, err);
}

}  // namespace

// ---- pcbenv_puct_move --------------------------------------------------------------------------------------------
// As pcbenv_puct_advance: every argument check before a device is touched, the null handle last; then one launch.
extern "C" int pcbenv_puct_move(const pcbenv *cenv, const pcbenv_puct_move_request *q) {
    using namespace pcb_tree_host;
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    PCB_TRY(check_request(env, q, "pcbenv_puct_move_request"));
    const int ph = q->phases;
    const bool choose = ph & PCBENV_MOVE_CHOOSE, reroot = ph & PCBENV_MOVE_REROOT;
    if (ph == 0 || (ph & ~(PCBENV_MOVE_CHOOSE | PCBENV_MOVE_REROOT)) != 0) return fail(env, PCBENV_EINVAL, "phases must be a non-empty set of CHOOSE, REROOT");
    if (choose && q->mode != PCBENV_MOVE_GREEDY && q->mode != PCBENV_MOVE_PROPORTIONAL) return fail(env, PCBENV_EINVAL, "unknown mode");
    PCB_TRY(check_extents(env, q));
    if (q->reserved != 0) return fail(env, PCBENV_EINVAL, "reserved must be 0");
    PCB_TRY(check_puct_tree(env, q));
    if (!q->move_slot) return fail(env, PCBENV_EINVAL, "null move_slot");
    if (choose && (!q->move_action || !q->child_visits || !q->child_actions || !q->root_value))
        return fail(env, PCBENV_EINVAL, "null move_action, child_visits, child_actions or root_value with CHOOSE");
    if (reroot && !q->remap) return fail(env, PCBENV_EINVAL, "null remap with REROOT");
    PCB_TRY(check_puct_doubles(env, q, choose ? q->root_value : 0));
    PCB_TREE_CHECKS_END(env, q);
    MoveArgs a;
    puct_tree_args(a, q);
    a.mode = q->mode; a.first_root = q->first_root; a.seed = q->seed; a.step_index = q->step_index;
    a.move_slot = q->move_slot; a.move_action = q->move_action; a.child_visits = q->child_visits; a.child_actions = q->child_actions;
    a.root_value = q->root_value; a.remap = q->remap; a.reset = q->reset;
    const unsigned grid = (unsigned)(((long long)a.P + BLOCK / LANES - 1) / (BLOCK / LANES));
    hipLaunchKernelGGL(k_puct_move, dim3(grid), dim3(BLOCK), 0, (hipStream_t)q->stream, a);
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}
